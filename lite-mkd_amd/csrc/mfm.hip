// MFM teacher-feature fusion (teacher/code/model.py:1135-1151,1300-1331,1361-1392,1648-1664), inference and training: the pieces of
// nn.TransformerEncoderLayer (post-norm, ReLU FFN) that are not GEMMs - LayerNorm (csrc/rows.h) and the attention over up to 8 tokens (and, in a
// second family, up to 16), forward and backward.  The GEMMs (in_proj, out_proj, linear1+ReLU, linear2, f1) run on lmkd_gemm_f32.  fp32, one workgroup per row / per
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

// ---- the second family: 1 <= L <= MS_L = 16 tokens (clips of 9 - 16 frames) ----
// 256 accumulators per thread do not fit, so the L x L reductions over the head dimension are split by query row: wave w of the 4 owns
// the rows 4w .. 4w+3 (4 x 16 = 64 accumulators per lane, as above), its 64 lanes stride over the head dimension, and one wave_sum per
// score finishes it - no sum across waves.  The 16 x 16 blocks (scores / P, P o M, dS and the two transposes the backward reads by
// row) live in LDS; the passes that write the head dimension (P V, dQ, dK, dV) run one thread per group of 4 elements with its 16
// tokens in registers.  Every loop over a private array is unrolled over 16 tokens with guards: none is indexed dynamically.
// A lane owns groups of 4 consecutive elements of the head dimension.  V4 (the head dimension a multiple of 4 and every buffer on a
// 16-byte boundary: the entry points decide) moves a group in one 16-byte access and works on it as one vector; otherwise the same code
// runs on one element at a time, in the same order, so both instances give the same bits.  At the real shapes there are fewer
// workgroups (150) than CUs, so the time depends on the bytes a wave keeps in flight: 20 rows x 16 bytes per lane in the reductions, 16
// rows in the other passes.
#define MS_L 16
#define MS_LL (MS_L * MS_L)
#define MS_ROWS 4      // query rows per wave
static_assert(MF_THREADS == MS_LL && MF_THREADS / 64 * MS_ROWS == MS_L, "one thread per score, 4 waves x 4 rows");

// the two element types, T = f32x4 (V4) or float: s + x . y ; o + m v ; c ? v : 0
__device__ __forceinline__ float ms_dot(float x, float y, float s) { return fmaf(x, y, s); }
__device__ __forceinline__ float ms_dot(const f32x4& x, const f32x4& y, float s) {
  return fmaf(x.w, y.w, fmaf(x.z, y.z, fmaf(x.y, y.y, fmaf(x.x, y.x, s))));
}
__device__ __forceinline__ float ms_axpy(float m, float v, float o) { return fmaf(m, v, o); }
__device__ __forceinline__ f32x4 ms_axpy(float m, const f32x4& v, const f32x4& o) {
  f32x4 r;
  r.x = fmaf(m, v.x, o.x);
  r.y = fmaf(m, v.y, o.y);
  r.z = fmaf(m, v.z, o.z);
  r.w = fmaf(m, v.w, o.w);
  return r;
}
__device__ __forceinline__ float ms_sel(bool c, float v) { return c ? v : 0.f; }
__device__ __forceinline__ f32x4 ms_sel(bool c, const f32x4& v) { return c ? v : f32x4{0.f, 0.f, 0.f, 0.f}; }

// rows[j] = row j of p (row stride ld) at element d, for N rows from j0; the rows beyond L read as zero.  Without a branch: a load under
// a condition is followed by a wait for it, which leaves one load in flight where there could be 20 (seen in the ISA: s_waitcnt vmcnt(0)
// after every guarded load).  So the address is clamped to the last row that exists and the load is unconditional; ms_zero_rows selects
// the zeros afterwards.  Between the two stands MS_PIN: an empty asm statement that names every loaded register as its operand, so it
// comes after all the loads and everything that uses them comes after it.  Left to itself the scheduler pairs each load with its first
// use and keeps 2 in flight (also seen in the ISA; __builtin_amdgcn_sched_barrier does not hold them: the uses move above it).
#define MS_PIN4(r) "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3])
#define MS_PIN16(r) MS_PIN4(r), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), \
                    "+v"(r[13]), "+v"(r[14]), "+v"(r[15])
template <class T, int N>
__device__ __forceinline__ void ms_ld_rows(T (&rows)[N], const float* __restrict__ p, int ld, int j0, int L, int d) {
#pragma unroll
  for (int j = 0; j < N; ++j) rows[j] = *reinterpret_cast<const T*>(p + (unsigned)(min(j0 + j, L - 1) * ld + d));      // unsigned: base + 32-bit offset addressing
}
template <class T, int N>
__device__ __forceinline__ void ms_zero_rows(T (&rows)[N], int j0, int L) {
#pragma unroll
  for (int j = 0; j < N; ++j) rows[j] = ms_sel(j0 + j < L, rows[j]);
}

// acc[i * 16 + j] += a[r0 + i, d] . b[j, d] over the elements of one T at d
template <class T>
__device__ __forceinline__ void ms_outer_step(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, int r0, int L, int d,
                                              float (&acc)[MS_ROWS * MS_L]) {
  T x[MS_ROWS], y[MS_L];
  ms_ld_rows(x, a, lda, r0, L, d);
  ms_ld_rows(y, b, ldb, 0, L, d);
  static_assert(MS_ROWS == 4 && MS_L == 16, "MS_PIN names 4 + 16 registers");
  asm volatile("" : MS_PIN4(x), MS_PIN16(y));      // all 20 loads are issued before anything waits for one
  ms_zero_rows(x, r0, L);
  ms_zero_rows(y, 0, L);
#pragma unroll
  for (int i = 0; i < MS_ROWS; ++i)
#pragma unroll
    for (int j = 0; j < MS_L; ++j) acc[i * MS_L + j] = ms_dot(x[i], y[j], acc[i * MS_L + j]);
}

// S[(4w + i) * 16 + j] = sum over the head dimension of a[4w + i, d] b[j, d]; rows and columns beyond L are zero.
// a / b: row 0 of the two operands at this head's first column, row strides lda / ldb.
template <bool V4>
__device__ __forceinline__ void ms_outer_sums(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, int L, int hd,
                                              float* __restrict__ S) {
  const int lane = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * MS_ROWS;
  float acc[MS_ROWS * MS_L];
#pragma unroll
  for (int e = 0; e < MS_ROWS * MS_L; ++e) acc[e] = 0.f;
  if (r0 < L) {      // wave-uniform: a wave whose rows all lie beyond L has nothing to sum
    for (int d0 = 4 * lane; d0 < hd; d0 += 4 * 64) {
      if constexpr (V4) {
        ms_outer_step<f32x4>(a, lda, b, ldb, r0, L, d0, acc);
      } else {
#pragma unroll 1
        for (int d = d0; d < min(d0 + 4, hd); ++d) ms_outer_step<float>(a, lda, b, ldb, r0, L, d, acc);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < MS_ROWS * MS_L; ++e) {
    const float v = wave_sum(acc[e]);
    if (lane == 0) S[r0 * MS_L + e] = v;
  }
}

// dst[i, d] = sum_j M[i * 16 + j] src[j, d] for the tokens i < L, over the elements of one T at d
template <class T>
__device__ __forceinline__ void ms_apply_at(const float* __restrict__ M, const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd,
                                            int L, int d) {
  T v[MS_L];
  ms_ld_rows(v, src, lds, 0, L, d);
  asm volatile("" : MS_PIN16(v));
  ms_zero_rows(v, 0, L);
  for (int i = 0; i < L; ++i) {
    T o = ms_sel(false, v[0]);
#pragma unroll
    for (int j = 0; j < MS_L; ++j) o = ms_axpy(M[i * MS_L + j], v[j], o);
    *reinterpret_cast<T*>(dst + i * ldd + d) = o;
  }
}

// the same for the whole head dimension: M a 16 x 16 block in LDS (zero beyond L), src / dst row 0 at this head's first column, row
// strides lds / ldd
template <bool V4>
__device__ __forceinline__ void ms_apply(const float* __restrict__ M, const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd,
                                         int L, int hd) {
  if constexpr (V4) {
#pragma unroll 1
    for (int d0 = 4 * threadIdx.x; d0 < hd; d0 += 4 * MF_THREADS) ms_apply_at<f32x4>(M, src, lds, dst, ldd, L, d0);
  } else {
#pragma unroll 1
    for (int d = threadIdx.x; d < hd; d += MF_THREADS) ms_apply_at<float>(M, src, lds, dst, ldd, L, d);
  }
}

template <bool KEEP, bool V4>
__global__ void __launch_bounds__(MF_THREADS) mha_seq_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ mask, float* __restrict__ out,
                                                                 float* __restrict__ Pout, int L, int D, int H, float scale) {
  __shared__ float P[MS_LL];
  __shared__ float PMk[KEEP ? MS_LL : 1];
  const float* PM = KEEP ? PMk : P;      // what meets V: P o mask, or P itself
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int hd = D / H;
  const float* base = qkv + (long)b * L * 3 * D + h * hd;
  ms_outer_sums<V4>(base, 3 * D, base + D, 3 * D, L, hd, P);
  __syncthreads();
  if (threadIdx.x < L) {      // one softmax row each, over its L columns
    const int i = threadIdx.x;
    float m = -INFINITY;
    for (int j = 0; j < L; ++j) { const float s = P[i * MS_L + j] * scale; P[i * MS_L + j] = s; m = fmaxf(m, s); }
    float z = 0.f;
    for (int j = 0; j < L; ++j) { const float e = expf(P[i * MS_L + j] - m); P[i * MS_L + j] = e; z += e; }
    for (int j = 0; j < L; ++j) P[i * MS_L + j] /= z;
  }
  __syncthreads();
  if constexpr (KEEP) {      // rows and columns beyond L hold the zero sums of their zero operands
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    const float p = P[threadIdx.x];
    Pout[(long)blockIdx.x * MS_LL + threadIdx.x] = p;
    PMk[threadIdx.x] = (mask && i < L && j < L) ? p * mask[((long)blockIdx.x * L + i) * L + j] : p;
    __syncthreads();
  }
  ms_apply<V4>(PM, base + 2 * D, 3 * D, out + (long)b * L * D + h * hd, D, L, hd);
}

// the 16-byte instances run where every group of 4 is whole and aligned
static bool mha_seq_v4(int D, int H, const void* a, const void* b, const void* c = nullptr) {
  return (D / H) % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(c);
}

static int mha_seq_check(const char* who, int B, int L, int D, int H) {
  LMKD_REQUIRE(B > 0 && H > 0, "%s: %d sequences, %d heads", who, B, H);
  LMKD_REQUIRE(L > 0 && L <= MS_L, "%s: %d tokens (1 to 16)", who, L);
  LMKD_REQUIRE(D > 0 && D % H == 0, "%s: width %d is no multiple of %d heads", who, D, H);
  LMKD_REQUIRE((long)MS_L * 3 * D <= 0x7fffffffL, "%s: width %d is past the 32-bit offsets inside one sequence", who, D);
  LMKD_REQUIRE((long)B * H <= 0x7fffffffL, "%s: %d x %d workgroups", who, B, H);
  return LMKD_OK;
}

extern "C" int lmkd_mha_seq(const float* qkv, float* out, int B, int L, int D, int H, void* stream) {
  if (int rc = mha_seq_check("lmkd_mha_seq", B, L, D, H)) return rc;
  LMKD_REQUIRE(qkv && out, "lmkd_mha_seq: null pointer");
  const auto kernel = mha_seq_v4(D, H, qkv, out) ? mha_seq_fwd_kernel<false, true> : mha_seq_fwd_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3(B * H), dim3(MF_THREADS), 0, (hipStream_t)stream, qkv, (const float*)nullptr, out, (float*)nullptr, L, D, H,
                     1.f / sqrtf((float)(D / H)));
  LMKD_CHECK_LAUNCH("mha_seq_fwd_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_mha_seq_train_fwd(const float* qkv, const float* mask, float* out, float* P, int B, int L, int D, int H, void* stream) {
  if (int rc = mha_seq_check("lmkd_mha_seq_train_fwd", B, L, D, H)) return rc;
  LMKD_REQUIRE(qkv && out && P, "lmkd_mha_seq_train_fwd: null pointer");
  const auto kernel = mha_seq_v4(D, H, qkv, out) ? mha_seq_fwd_kernel<true, true> : mha_seq_fwd_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3(B * H), dim3(MF_THREADS), 0, (hipStream_t)stream, qkv, mask, out, P, L, D, H, 1.f / sqrtf((float)(D / H)));
  LMKD_CHECK_LAUNCH("mha_seq_fwd_kernel");
  return LMKD_OK;
}

// Backward per (sequence, head), the formulas of mha_small_bwd_kernel.  dS and P o M are kept transposed too, so that the last pass
// reads every operand of dK and dV along a row of LDS.
template <bool V4>
__global__ void __launch_bounds__(MF_THREADS) mha_seq_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ Pg, const float* __restrict__ mask,
                                                                 const float* __restrict__ dO, float* __restrict__ dqkv, int L, int D, int H, float scale) {
  __shared__ float Ps[MS_LL];       // P
  __shared__ float PMT[MS_LL];      // (P o M)^T
  __shared__ float dS[MS_LL];       // dO V^T, then dP, then dS
  __shared__ float dST[MS_LL];      // dS^T
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int hd = D / H;
  const float* base = qkv + (long)b * L * 3 * D + h * hd;
  const float* gb = dO + (long)b * L * D + h * hd;
  ms_outer_sums<V4>(gb, D, base + 2 * D, 3 * D, L, hd, dS);
  __syncthreads();
  {
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    const bool in = i < L && j < L;
    const float m = (mask && in) ? mask[((long)blockIdx.x * L + i) * L + j] : 1.f;
    const float p = in ? Pg[(long)blockIdx.x * MS_LL + threadIdx.x] : 0.f;      // P is zero beyond L
    Ps[threadIdx.x] = p;
    PMT[j * MS_L + i] = p * m;
    dS[threadIdx.x] *= m;
  }
  __syncthreads();
  if (threadIdx.x < MS_L) {      // one softmax row each; P is zero beyond L, so are these rows' and columns' dS
    const int i = threadIdx.x;
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < MS_L; ++j) r = fmaf(dS[i * MS_L + j], Ps[i * MS_L + j], r);
#pragma unroll
    for (int j = 0; j < MS_L; ++j) {
      const float s = Ps[i * MS_L + j] * (dS[i * MS_L + j] - r) * scale;
      dS[i * MS_L + j] = s;
      dST[j * MS_L + i] = s;
    }
  }
  __syncthreads();
  float* ob = dqkv + (long)b * L * 3 * D + h * hd;
  ms_apply<V4>(dS, base + D, 3 * D, ob, 3 * D, L, hd);              // dQ[i] = sum_j dS[i, j] K[j]
  ms_apply<V4>(dST, base, 3 * D, ob + D, 3 * D, L, hd);             // dK[i] = sum_j dS[j, i] Q[j]
  ms_apply<V4>(PMT, gb, D, ob + 2 * D, 3 * D, L, hd);               // dV[i] = sum_j (P o M)[j, i] dO[j]
}

extern "C" int lmkd_mha_seq_bwd(const float* qkv, const float* P, const float* mask, const float* dO, float* dqkv, int B, int L, int D,
                                int H, void* stream) {
  if (int rc = mha_seq_check("lmkd_mha_seq_bwd", B, L, D, H)) return rc;
  LMKD_REQUIRE(qkv && P && dO && dqkv, "lmkd_mha_seq_bwd: null pointer");
  const auto kernel = mha_seq_v4(D, H, qkv, dO, dqkv) ? mha_seq_bwd_kernel<true> : mha_seq_bwd_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(B * H), dim3(MF_THREADS), 0, (hipStream_t)stream, qkv, P, mask, dO, dqkv, L, D, H,
                     1.f / sqrtf((float)(D / H)));
  LMKD_CHECK_LAUNCH("mha_seq_bwd_kernel");
  return LMKD_OK;
}
