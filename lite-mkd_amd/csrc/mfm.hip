// MFM teacher-feature fusion (teacher/code/model.py:1135-1151,1300-1331,1361-1392,1648-1664), inference and training: the pieces of
// nn.TransformerEncoderLayer (post-norm, ReLU FFN) that are not GEMMs - LayerNorm (csrc/rows.h) and the 8-token attention, forward and
// backward.  The GEMMs (in_proj, out_proj, linear1+ReLU, linear2, f1) run on lmkd_gemm_f32.  fp32, one workgroup per row / per
// (sequence, head), every sum in a fixed order: no atomics, two calls give the same bits.
#include "rows.h"

#define MF_THREADS ROW_THREADS

// y[r, col_off : col_off+D] (row stride ldy) = LayerNorm(x[r,:] (+ res[r % res_rows, :])) * gamma + beta
extern "C" int lmkd_layernorm_fwd(const float* x, const float* res, long res_rows, const float* gamma, const float* beta, float* y,
                                  long ldy, long rows, int D, float eps, void* stream) {
  LMKD_REQUIRE(x && gamma && beta && y && rows > 0 && D > 0 && ldy >= D, "lmkd_layernorm_fwd: bad arguments");
  LMKD_REQUIRE(!res || res_rows > 0, "lmkd_layernorm_fwd: res_rows must be positive");
  LMKD_REQUIRE((size_t)D * sizeof(float) <= 96 * 1024, "lmkd_layernorm_fwd: row of %d floats does not fit in LDS", D);
  hipLaunchKernelGGL((ln_fwd_kernel<true, false>), dim3((unsigned)rows), dim3(ROW_THREADS), (size_t)D * sizeof(float), (hipStream_t)stream, x,
                     res, res_rows, gamma, beta, (const float*)nullptr, y, ldy, (float*)nullptr, (float*)nullptr, D, eps);
  LMKD_CHECK_LAUNCH("ln_fwd_kernel");
  return LMKD_OK;
}

// the same with what the backward reads, xhat [rows, D] and rstd [rows] (model.py:1143-1151 TrainablePositionalEncoding.forward,
// :1317-1323 ThreeTransforTemproal.forward, :1376-1385 TwoTransforFusion.forward); y *= mask[r, :] (the dropout of :1150; nullable)
extern "C" int lmkd_layernorm_train_fwd(const float* x, const float* res, long res_rows, const float* gamma, const float* beta,
                                        const float* mask, float* y, long ldy, float* xhat, float* rstd, long rows, int D, float eps,
                                        void* stream) {
  LMKD_REQUIRE(rows > 0 && D > 0, "lmkd_layernorm_train_fwd: %ld rows of %d", rows, D);
  LMKD_REQUIRE(ldy >= D, "lmkd_layernorm_train_fwd: output row stride %ld below the row length %d", ldy, D);
  LMKD_REQUIRE(!res || res_rows > 0, "lmkd_layernorm_train_fwd: res_rows must be positive");
  LMKD_REQUIRE((size_t)D * sizeof(float) <= 96 * 1024, "lmkd_layernorm_train_fwd: row of %d floats does not fit in LDS", D);
  LMKD_REQUIRE(x && gamma && beta && y && xhat && rstd, "lmkd_layernorm_train_fwd: null pointer");
  hipLaunchKernelGGL((ln_fwd_kernel<true, true>), dim3((unsigned)rows), dim3(ROW_THREADS), (size_t)D * sizeof(float), (hipStream_t)stream, x,
                     res, res_rows, gamma, beta, mask, y, ldy, xhat, rstd, D, eps);
  LMKD_CHECK_LAUNCH("ln_fwd_kernel");
  return LMKD_OK;
}

// dpre[r, :] = the gradient of that LayerNorm's input from dy[r, :] (row stride lddy) ; dyc[r, :] = dy[r, :] o mask[r, :] (nullable), the
// operand of the dgamma / dbeta column sums
extern "C" int lmkd_layernorm_train_bwd(const float* dy, long lddy, const float* mask, const float* xhat, const float* rstd,
                                        const float* gamma, float* dpre, float* dyc, long rows, int D, void* stream) {
  LMKD_REQUIRE(rows > 0 && D > 0, "lmkd_layernorm_train_bwd: %ld rows of %d", rows, D);
  LMKD_REQUIRE(lddy >= D, "lmkd_layernorm_train_bwd: gradient row stride %ld below the row length %d", lddy, D);
  LMKD_REQUIRE((size_t)D * sizeof(float) <= 96 * 1024, "lmkd_layernorm_train_bwd: row of %d floats is past the forward's limit", D);
  LMKD_REQUIRE(dy && xhat && rstd && gamma && dpre, "lmkd_layernorm_train_bwd: null pointer");
  LMKD_REQUIRE(dpre != dy && dyc != dy, "lmkd_layernorm_train_bwd: the outputs may not alias dy (it is read twice)");
  hipLaunchKernelGGL(ln_bwd_kernel<false>, dim3((unsigned)rows), dim3(ROW_THREADS), 0, (hipStream_t)stream, dy, lddy, mask, xhat, rstd, gamma, dpre,
                     dyc, D);
  LMKD_CHECK_LAUNCH("ln_bwd_kernel");
  return LMKD_OK;
}

// Self-attention over L <= 8 tokens per (sequence, head): qkv [B*L, 3*D] (q | k | v), out [B*L, D], head dim hd = D/H.
// KEEP (training) keeps the probabilities: Pout [B*H, 8, 8] (before dropout; zero beyond L), and multiplies them by mask [B*H, L, L]
// (nullable) on their way to V - the dropout inside nn.MultiheadAttention.  The loops over private arrays are unrolled over 8 tokens
// (with guards where they load): none is indexed dynamically.
template <bool KEEP>
__global__ void mha_small_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ mask, float* __restrict__ out,
                                     float* __restrict__ Pout, int L, int D, int H, float scale) {
  __shared__ float part[4][64];
  __shared__ float P[64];
  __shared__ float PMk[KEEP ? 64 : 1];
  const float* PM = KEEP ? PMk : P;      // what meets V: P o mask, or P itself
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int hd = D / H;
  const float* base = qkv + (long)b * L * 3 * D + h * hd;
  float acc[64];
#pragma unroll
  for (int e = 0; e < 64; ++e) acc[e] = 0.f;
  for (int d = threadIdx.x; d < hd; d += MF_THREADS) {
    float q[8], k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      q[i] = i < L ? base[(long)i * 3 * D + d] : 0.f;
      k[i] = i < L ? base[(long)i * 3 * D + D + d] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i * 8 + j] = fmaf(q[i], k[j], acc[i * 8 + j]);
  }
#pragma unroll
  for (int e = 0; e < 64; ++e) {
    const float v = wave_sum(acc[e]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) P[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]) * scale;
  __syncthreads();
  if (threadIdx.x < L) {
    const int i = threadIdx.x;
    float m = -INFINITY;
    for (int j = 0; j < L; ++j) m = fmaxf(m, P[i * 8 + j]);
    float z = 0.f;
    for (int j = 0; j < L; ++j) { const float e = expf(P[i * 8 + j] - m); P[i * 8 + j] = e; z += e; }
    for (int j = 0; j < L; ++j) P[i * 8 + j] /= z;
  }
  __syncthreads();
  if constexpr (KEEP) {
    if (threadIdx.x < 64) {      // rows and columns beyond L hold the zero scores of their zero operands
      const int i = threadIdx.x >> 3, j = threadIdx.x & 7;
      const float p = P[threadIdx.x];
      Pout[(long)blockIdx.x * 64 + threadIdx.x] = p;
      PMk[threadIdx.x] = (mask && i < L && j < L) ? p * mask[((long)blockIdx.x * L + i) * L + j] : p;
    }
    __syncthreads();
  }
  float* ob = out + (long)b * L * D + h * hd;
  for (int d = threadIdx.x; d < hd; d += MF_THREADS) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < L ? base[(long)j * 3 * D + 2 * D + d] : 0.f;
    for (int i = 0; i < L; ++i) {
      float o = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) o = fmaf(PM[i * 8 + j], v[j], o);
      ob[(long)i * D + d] = o;
    }
  }
}

extern "C" int lmkd_mha_small(const float* qkv, float* out, int B, int L, int D, int H, void* stream) {
  LMKD_REQUIRE(qkv && out && B > 0 && L > 0 && L <= 8 && H > 0 && D % H == 0, "lmkd_mha_small: bad arguments (L <= 8)");
  hipLaunchKernelGGL(mha_small_fwd_kernel<false>, dim3(B * H), dim3(MF_THREADS), 0, (hipStream_t)stream, qkv, (const float*)nullptr, out,
                     (float*)nullptr, L, D, H, 1.f / sqrtf((float)(D / H)));
  LMKD_CHECK_LAUNCH("mha_small_fwd_kernel");
  return LMKD_OK;
}

static int mha_small_check(const char* who, int B, int L, int D, int H) {
  LMKD_REQUIRE(B > 0 && H > 0, "%s: %d sequences, %d heads", who, B, H);
  LMKD_REQUIRE(L > 0 && L <= 8, "%s: %d tokens (1 to 8)", who, L);
  LMKD_REQUIRE(D > 0 && D % H == 0, "%s: width %d is no multiple of %d heads", who, D, H);
  LMKD_REQUIRE((long)B * H <= 0x7fffffffL, "%s: %d x %d workgroups", who, B, H);
  return LMKD_OK;
}

extern "C" int lmkd_mha_small_train_fwd(const float* qkv, const float* mask, float* out, float* P, int B, int L, int D, int H,
                                        void* stream) {
  if (int rc = mha_small_check("lmkd_mha_small_train_fwd", B, L, D, H)) return rc;
  LMKD_REQUIRE(qkv && out && P, "lmkd_mha_small_train_fwd: null pointer");
  hipLaunchKernelGGL(mha_small_fwd_kernel<true>, dim3(B * H), dim3(MF_THREADS), 0, (hipStream_t)stream, qkv, mask, out, P, L, D, H,
                     1.f / sqrtf((float)(D / H)));
  LMKD_CHECK_LAUNCH("mha_small_fwd_kernel");
  return LMKD_OK;
}

// Backward per (sequence, head).  The 64 sums dO V^T over the head dimension are reduced as the forward reduces Q K^T: per wave, then
// across the 4 waves in fixed order.  Every loop over the tokens is unrolled over 8 with guards: no private array is indexed dynamically.
__global__ void __launch_bounds__(MF_THREADS) mha_small_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ Pg, const float* __restrict__ mask,
                                     const float* __restrict__ dO, float* __restrict__ dqkv, int L, int D, int H, float scale) {
  __shared__ float part[4][64];
  __shared__ float Ps[64];      // P
  __shared__ float PM[64];      // P o M
  __shared__ float dS[64];      // dP, then dS
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int hd = D / H;
  const float* base = qkv + (long)b * L * 3 * D + h * hd;
  const float* gb = dO + (long)b * L * D + h * hd;
  float acc[64];
#pragma unroll
  for (int e = 0; e < 64; ++e) acc[e] = 0.f;
  for (int d = threadIdx.x; d < hd; d += MF_THREADS) {
    float g[8], v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      g[i] = i < L ? gb[(long)i * D + d] : 0.f;
      v[i] = i < L ? base[(long)i * 3 * D + 2 * D + d] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i * 8 + j] = fmaf(g[i], v[j], acc[i * 8 + j]);
  }
#pragma unroll
  for (int e = 0; e < 64; ++e) {
    const float v = wave_sum(acc[e]);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int i = threadIdx.x >> 3, j = threadIdx.x & 7;
    const float m = (mask && i < L && j < L) ? mask[((long)blockIdx.x * L + i) * L + j] : 1.f;
    const float p = Pg[(long)blockIdx.x * 64 + threadIdx.x];
    Ps[threadIdx.x] = p;
    PM[threadIdx.x] = p * m;
    dS[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]) * m;
  }
  __syncthreads();
  if (threadIdx.x < 8) {      // one softmax row each; P is zero beyond L, so are these rows' and columns' dS
    const int i = threadIdx.x;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) r = fmaf(dS[i * 8 + j], Ps[i * 8 + j], r);
#pragma unroll
    for (int j = 0; j < 8; ++j) dS[i * 8 + j] = Ps[i * 8 + j] * (dS[i * 8 + j] - r) * scale;
  }
  __syncthreads();
  float* ob = dqkv + (long)b * L * 3 * D + h * hd;
  for (int d = threadIdx.x; d < hd; d += MF_THREADS) {
    float q[8], k[8], g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      q[i] = i < L ? base[(long)i * 3 * D + d] : 0.f;
      k[i] = i < L ? base[(long)i * 3 * D + D + d] : 0.f;
      g[i] = i < L ? gb[(long)i * D + d] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float dq = 0.f, dk = 0.f, dv = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dq = fmaf(dS[i * 8 + j], k[j], dq);      // dQ[i] = sum_j dS[i, j] K[j]
        dk = fmaf(dS[j * 8 + i], q[j], dk);      // dK[i] = sum_j dS[j, i] Q[j]
        dv = fmaf(PM[j * 8 + i], g[j], dv);      // dV[i] = sum_j (P o M)[j, i] dO[j]
      }
      if (i < L) {
        ob[(long)i * 3 * D + d] = dq;
        ob[(long)i * 3 * D + D + d] = dk;
        ob[(long)i * 3 * D + 2 * D + d] = dv;
      }
    }
  }
}

extern "C" int lmkd_mha_small_bwd(const float* qkv, const float* P, const float* mask, const float* dO, float* dqkv, int B, int L, int D,
                                  int H, void* stream) {
  if (int rc = mha_small_check("lmkd_mha_small_bwd", B, L, D, H)) return rc;
  LMKD_REQUIRE(qkv && P && dO && dqkv, "lmkd_mha_small_bwd: null pointer");
  hipLaunchKernelGGL(mha_small_bwd_kernel, dim3(B * H), dim3(MF_THREADS), 0, (hipStream_t)stream, qkv, P, mask, dO, dqkv, L, D, H,
                     1.f / sqrtf((float)(D / H)));
  LMKD_CHECK_LAUNCH("mha_small_bwd_kernel");
  return LMKD_OK;
}
