// OTAM matcher head (reference: teacher/code/model.py:3260-3343 cos_sim, OTAM_cum_dist, CNN_OTAM): frame cosine distances, the ordered
// temporal alignment table in both directions per (query, support) pair, class means and the softmax - DESIGN.md 17.
//
// The soft minimum -l log sum exp(-a / l), l = 0.1, is evaluated after its minimum is subtracted: m - l log sum exp(-(a - m) / l).  Equal
// to the reference's form wherever that one is finite, and finite where exp(-a / 0.1) underflows in fp32 (a beyond about 10.4: every
// seq_len >= 12 with unrelated features).
//
// Table of one direction over the L x L block B of frame distances, P = B with one zero column on each side (columns 0 .. L+1):
//   row 0:   C[0][m] = P[0][m] + C[0][m-1]                        (a running sum), C[.][0] = 0 everywhere (never stored)
//   row l:   C[l][1]   = P[l][1] + softmin(0, C[l-1][1], 0)
//            C[l][m]   = P[l][m] + softmin(C[l-1][m-1], C[l][m-1])           m = 2 .. L
//            C[l][L+1] =           softmin(C[l-1][L], C[l-1][L+1], C[l][L])
// value C[L-1][L+1]; direction A runs on B (query frame = row), direction B on its transpose; cum = A + B.
// Stored cells: columns 1 .. L+1 of every row, cell (l, m) at l (L+1) + m-1.
#include "common.h"
#include <atomic>

// the LDS instance keeps run-time loop bounds: its `#pragma unroll`s are requests the register instance needs and this one cannot take
#pragma clang diagnostic ignored "-Wpass-failed"

#define OT_MAX_L 16
#define OT_MAX_NS 512
#define OT_INV_LBDA 10.f
#define OT_LBDA 0.1f
#define OT_EPS 0.01f
#define OT_REG_L 8                 // the instance with the table in registers
#define OT_REG_LANES 512           // ... for at most 256 support videos: 512 lanes leave each wave 256 registers
#define OT_LDS_BUDGET (128 * 1024) // dynamic LDS of the generic path (of 160 KB; the reductions' static arrays come on top)

extern "C" int lmkd_gemm_f32(char layA, char layB, int M, int N, int K, float alpha, const float* A, long lda, long sA, const float* B,
                             long ldb, long sB, float beta, float* C, long ldc, long sC, const float* bias, int relu, int batch,
                             void* stream);

static inline long ot_ldd(int Ns, int L) { return ((long)Ns * L + 3) & ~3L; }

// ---------------------------------------------------------------------------------
// frame distances
// ---------------------------------------------------------------------------------
// one wave per row of [X; Y]: r = |row|
__global__ __launch_bounds__(256) void otam_norms_kernel(const float4* __restrict__ X, const float4* __restrict__ Y, float* __restrict__ rq,
                                                         float* __restrict__ rs, int Mq, int Ms, int D4) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Mq + Ms) return;
  const float4* p = row < Mq ? X + (long)row * D4 : Y + (long)(row - Mq) * D4;
  float acc = 0.f;
  for (int i = lane; i < D4; i += 64) {
    const float4 v = p[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  acc = wave_sum(acc);
  if (lane == 0) (row < Mq ? rq[row] : rs[row - Mq]) = sqrtf(acc);
}

// d = 1 - n / (rq rs + 0.01) over [Mq, ldd]; the pad columns (j >= Ms) hold 0
__global__ __launch_bounds__(256) void otam_dist_kernel(const float* __restrict__ n, const float* __restrict__ rq, const float* __restrict__ rs,
                                                        float* __restrict__ dist, int Mq, int Ms, int ldd) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Mq * ldd) return;
  const int r = (int)(i / ldd), j = (int)(i - (long)r * ldd);
  dist[i] = j < Ms ? 1.f - n[i] / (rq[r] * rs[j] + OT_EPS) : 0.f;
}

static int ot_check_dims(const char* who, int Nq, int Ns, int L, int D) {
  LMKD_REQUIRE(L >= 1 && L <= OT_MAX_L, "%s: seq_len %d outside 1 .. %d", who, L, OT_MAX_L);
  LMKD_REQUIRE(Ns >= 1 && Ns <= OT_MAX_NS, "%s: %d support videos outside 1 .. %d", who, Ns, OT_MAX_NS);
  LMKD_REQUIRE(Nq >= 1 && (long)Nq * L * ot_ldd(Ns, L) < (1L << 31), "%s: %d queries", who, Nq);
  LMKD_REQUIRE(D >= 4 && D % 4 == 0, "%s: D = %d is not a positive multiple of 4", who, D);
  return LMKD_OK;
}

extern "C" int lmkd_otam_frame_dist_fwd(const float* X, const float* Y, float* n, float* rq, float* rs, float* dist, int Nq, int Ns, int L,
                                        int D, void* stream) {
  if (int rc = ot_check_dims("lmkd_otam_frame_dist_fwd", Nq, Ns, L, D)) return rc;
  LMKD_REQUIRE(X && Y && n && rq && rs && dist, "lmkd_otam_frame_dist_fwd: null pointer");
  LMKD_REQUIRE(aligned16(X) && aligned16(Y), "lmkd_otam_frame_dist_fwd: the frame matrices must be 16-byte aligned");
  const int Mq = Nq * L, Ms = Ns * L;
  const long ldd = ot_ldd(Ns, L);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = lmkd_gemm_f32('K', 'K', Mq, Ms, D, 1.f, X, D, 0, Y, D, 0, 0.f, n, ldd, 0, nullptr, 0, 1, stream)) return rc;
  hipLaunchKernelGGL(otam_norms_kernel, dim3(cdiv(Mq + Ms, 4)), dim3(256), 0, st, (const float4*)X, (const float4*)Y, rq, rs, Mq, Ms, D / 4);
  hipLaunchKernelGGL(otam_dist_kernel, dim3(cdiv((long)Mq * ldd, 256)), dim3(256), 0, st, (const float*)n, (const float*)rq, (const float*)rs,
                     dist, Mq, Ms, (int)ldd);
  LMKD_CHECK_LAUNCH("lmkd_otam_frame_dist_fwd");
  return LMKD_OK;
}

// Blocks 0 .. Mq-1: query frame i - Gd[i][j] = g / den (g = d loss / d sim = -dD, den = rq rs + 0.01; pad columns 0), the coefficient
// sum_j g n rs / den^2, and dQ[i] = -coefficient / rq x_i (0 for a frame of norm 0): the term the GEMM then accumulates onto.
// Blocks Mq .. Mq+ldd-1: support frame j the same down its column (pad rows: dS = 0).
__global__ __launch_bounds__(256) void otam_dist_bwd_kernel(const float* __restrict__ dD, const float* __restrict__ n, const float* __restrict__ rq,
                                                            const float* __restrict__ rs, const float4* __restrict__ X,
                                                            const float4* __restrict__ Y, float* __restrict__ Gd, float4* __restrict__ dQ,
                                                            float4* __restrict__ dS, int Mq, int Ms, int ldd, int D4) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  float acc = 0.f;
  if (b < Mq) {
    const float r = rq[b];
    for (int j = threadIdx.x; j < ldd; j += 256) {
      float gd = 0.f;
      if (j < Ms) {
        const float den = r * rs[j] + OT_EPS;
        gd = -dD[(long)b * ldd + j] / den;
        acc += gd * n[(long)b * ldd + j] * rs[j] / den;
      }
      Gd[(long)b * ldd + j] = gd;
    }
    acc = block_sum_256(acc, red);
    const float sc = r > 0.f ? -acc / r : 0.f;
    for (int i = threadIdx.x; i < D4; i += 256) {
      const float4 v = X[(long)b * D4 + i];
      dQ[(long)b * D4 + i] = make_float4(sc * v.x, sc * v.y, sc * v.z, sc * v.w);
    }
    return;
  }
  const int j = b - Mq;
  if (j >= Ms) {
    for (int i = threadIdx.x; i < D4; i += 256) dS[(long)j * D4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float r = rs[j];
  for (int i = threadIdx.x; i < Mq; i += 256) {
    const float den = rq[i] * r + OT_EPS;
    acc += -dD[(long)i * ldd + j] / den * n[(long)i * ldd + j] * rq[i] / den;
  }
  acc = block_sum_256(acc, red);
  const float sc = r > 0.f ? -acc / r : 0.f;
  for (int i = threadIdx.x; i < D4; i += 256) {
    const float4 v = Y[(long)j * D4 + i];
    dS[(long)j * D4 + i] = make_float4(sc * v.x, sc * v.y, sc * v.z, sc * v.w);
  }
}

extern "C" int lmkd_otam_frame_dist_bwd(const float* dD, const float* X, const float* Y, const float* n, const float* rq, const float* rs,
                                        float* Gd, float* dQ, float* dS, int Nq, int Ns, int L, int D, void* stream) {
  if (int rc = ot_check_dims("lmkd_otam_frame_dist_bwd", Nq, Ns, L, D)) return rc;
  LMKD_REQUIRE(dD && X && Y && n && rq && rs && Gd && dQ && dS, "lmkd_otam_frame_dist_bwd: null pointer");
  LMKD_REQUIRE(aligned16(X) && aligned16(Y) && aligned16(Gd) && aligned16(dQ) && aligned16(dS), "lmkd_otam_frame_dist_bwd: 16-byte alignment");
  const int Mq = Nq * L, Ms = Ns * L;
  const int ldd = (int)ot_ldd(Ns, L);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(otam_dist_bwd_kernel, dim3(Mq + ldd), dim3(256), 0, st, dD, n, rq, rs, (const float4*)X, (const float4*)Y, Gd, (float4*)dQ,
                     (float4*)dS, Mq, Ms, ldd, D / 4);
  LMKD_CHECK_LAUNCH("lmkd_otam_frame_dist_bwd");
  // dQ += Gd Y over K = ldd (Gd's pad columns and Y's pad rows are 0);  dS += Gd^T X over its ldd rows
  if (int rc = lmkd_gemm_f32('K', 'N', Mq, D, ldd, 1.f, Gd, ldd, 0, Y, D, 0, 1.f, dQ, D, 0, nullptr, 0, 1, stream)) return rc;
  return lmkd_gemm_f32('M', 'N', ldd, D, Mq, 1.f, Gd, ldd, 0, X, D, 0, 1.f, dS, D, 0, nullptr, 0, 1, stream);
}

// ---------------------------------------------------------------------------------
// alignment
// ---------------------------------------------------------------------------------
__host__ __device__ __forceinline__ float ot_softmin2(float a, float b) {
  const float m = fminf(a, b);
  return m - OT_LBDA * logf(expf(-(a - m) * OT_INV_LBDA) + expf(-(b - m) * OT_INV_LBDA));
}
__host__ __device__ __forceinline__ float ot_softmin3(float a, float b, float c) {
  const float m = fminf(fminf(a, b), c);
  return m - OT_LBDA * logf(expf(-(a - m) * OT_INV_LBDA) + expf(-(b - m) * OT_INV_LBDA) + expf(-(c - m) * OT_INV_LBDA));
}
// share of a soft minimum's gradient that predecessor `a` takes: exp(-(a - softmin) / l)
__host__ __device__ __forceinline__ float ot_w(float a, float smv) { return expf(-(a - smv) * OT_INV_LBDA); }

// The table of one lane: LT > 0 in registers (every index a compile-time constant once the loops are unrolled), LT = 0 in LDS laid out
// [cell][lane] - consecutive lanes on consecutive banks.  C(l, m): table cell, m = 1 .. L+1; E(r, m): the two rolling rows of the backward.
template <int LT>
struct OtTab {
  float c[LT * (LT + 1)];
  float e[2][LT + 1];
  __host__ __device__ __forceinline__ float& C(int l, int m) { return c[l * (LT + 1) + m - 1]; }
  __host__ __device__ __forceinline__ float& E(int r, int m) { return e[r][m - 1]; }
};
template <>
struct OtTab<0> {
  float* base;
  int stride, L;
  __host__ __device__ __forceinline__ float& C(int l, int m) { return base[(l * (L + 1) + m - 1) * stride]; }
  __host__ __device__ __forceinline__ float& E(int r, int m) { return base[((L + r) * (L + 1) + m - 1) * stride]; }
};
static inline int ot_cells(int L) { return (L + 2) * (L + 1); }

// P[l][m] = pb[l sl + (m-1) sm], m = 1 .. L
template <int LT, class Tab>
__host__ __device__ __forceinline__ float ot_fill(Tab& T, const float* __restrict__ pb, long sl, long sm, int Lrt) {
  const int L = LT ? LT : Lrt;
  float run = 0.f;
#pragma unroll
  for (int m = 1; m <= L; ++m) {
    run += pb[(m - 1) * sm];
    T.C(0, m) = run;
  }
  T.C(0, L + 1) = run;
#pragma unroll
  for (int l = 1; l < L; ++l) {
    const float* pr = pb + l * sl;
    float left = pr[0] + ot_softmin3(0.f, T.C(l - 1, 1), 0.f);
    T.C(l, 1) = left;
#pragma unroll
    for (int m = 2; m <= L; ++m) {
      left = pr[(m - 1) * sm] + ot_softmin2(T.C(l - 1, m - 1), left);
      T.C(l, m) = left;
    }
    T.C(l, L + 1) = ot_softmin3(T.C(l - 1, L), T.C(l - 1, L + 1), left);
  }
  return T.C(L - 1, L + 1);
}

// E recursion over a filled table, seeded with gs at (L-1, L+1); on return C(l, m), m = 1 .. L, holds d value / d P[l][m]
template <int LT, class Tab>
__host__ __device__ __forceinline__ void ot_back(Tab& T, const float* __restrict__ pb, long sl, long sm, int Lrt, float gs) {
  const int L = LT ? LT : Lrt;
#pragma unroll
  for (int m = 1; m <= L; ++m) T.E((L - 1) & 1, m) = 0.f;
  T.E((L - 1) & 1, L + 1) = gs;
#pragma unroll
  for (int l = L - 1; l >= 1; --l) {
    const int cur = l & 1, prv = cur ^ 1;
    const float* pr = pb + l * sl;
#pragma unroll
    for (int m = 1; m <= L + 1; ++m) T.E(prv, m) = 0.f;
    {
      const float e = T.E(cur, L + 1), smv = T.C(l, L + 1);
      T.E(prv, L) += e * ot_w(T.C(l - 1, L), smv);
      T.E(prv, L + 1) += e * ot_w(T.C(l - 1, L + 1), smv);
      T.E(cur, L) += e * ot_w(T.C(l, L), smv);
      T.C(l, L + 1) = e;
    }
#pragma unroll
    for (int m = L; m >= 2; --m) {
      const float e = T.E(cur, m), smv = T.C(l, m) - pr[(m - 1) * sm];
      T.E(prv, m - 1) += e * ot_w(T.C(l - 1, m - 1), smv);
      T.E(cur, m - 1) += e * ot_w(T.C(l, m - 1), smv);
      T.C(l, m) = e;
    }
    {
      const float e = T.E(cur, 1), smv = T.C(l, 1) - pr[0];
      T.E(prv, 1) += e * ot_w(T.C(l - 1, 1), smv);
      T.C(l, 1) = e;
    }
  }
#pragma unroll
  for (int m = L + 1; m >= 2; --m) {
    const float e = T.E(0, m);
    T.E(0, m - 1) += e;
    T.C(0, m) = e;
  }
  T.C(0, 1) = T.E(0, 1);
}

// One workgroup per query.  Pair-direction t: support t >> 1, direction t & 1 (0: rows = query frames).  The register instance has one
// lane per pair-direction; the LDS instance walks the 2 Ns pair-directions in rounds of blockDim.x (as many lanes as its table space holds).
template <int LT>
__global__ __launch_bounds__(LT ? OT_REG_LANES : 1024) void otam_align_fwd_kernel(const float* __restrict__ dist, const int* __restrict__ cls,
                                                                                  float* __restrict__ cum, float* __restrict__ logits, int Ns,
                                                                                  int way, int Lrt, int ldd) {
  extern __shared__ float ot_lds[];
  __shared__ float sv[2 * OT_MAX_NS];
  __shared__ float scd[OT_MAX_NS];
  const int L = LT ? LT : Lrt, q = blockIdx.x;
  for (int t0 = 0; t0 < 2 * Ns; t0 += blockDim.x) {
    const int t = t0 + threadIdx.x;
    if (t < 2 * Ns) {
      const int s = t >> 1, dir = t & 1;
      const float* pb = dist + (long)q * L * ldd + (long)s * L;
      OtTab<LT> T;
      if constexpr (LT == 0) { T.base = ot_lds + threadIdx.x; T.stride = blockDim.x; T.L = L; }
      sv[t] = ot_fill<LT>(T, pb, dir ? 1 : ldd, dir ? ldd : 1, L);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < Ns; s += blockDim.x) cum[(long)q * Ns + s] = sv[2 * s] + sv[2 * s + 1];
  // class means in support order, then the softmax of their negatives: every sum in a fixed order
  for (int c = threadIdx.x; c < way; c += blockDim.x) {
    float a = 0.f;
    int k = 0;
    for (int s = 0; s < Ns; ++s)
      if (cls[s] == c) { a += sv[2 * s] + sv[2 * s + 1]; ++k; }
    scd[c] = k ? -a / (float)k : 0.f;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < way; c += blockDim.x) {
    float mx = scd[0], sum = 0.f;
    for (int k = 1; k < way; ++k) mx = fmaxf(mx, scd[k]);
    for (int k = 0; k < way; ++k) sum += expf(scd[k] - mx);
    logits[(long)q * way + c] = expf(scd[c] - mx) / sum;
  }
}

template <int LT>
__global__ __launch_bounds__(LT ? OT_REG_LANES : 1024) void otam_align_bwd_kernel(const float* __restrict__ dist, const int* __restrict__ cls,
                                                                                  const float* __restrict__ logits, const float* __restrict__ dlogits,
                                                                                  float* __restrict__ dD, int Ns, int way, int Lrt, int ldd) {
  extern __shared__ float ot_lds[];
  __shared__ float sg[OT_MAX_NS];      // d loss / d class distance over the class's count, per class
  const int L = LT ? LT : Lrt, q = blockIdx.x;
  // softmax backward: z = -cd, dz_c = p_c (dl_c - sum_k dl_k p_k); d cd_c = -dz_c; each of the class's supports takes 1 / count of it
  for (int c = threadIdx.x; c < way; c += blockDim.x) {
    float dot = 0.f;
    for (int k = 0; k < way; ++k) dot += dlogits[(long)q * way + k] * logits[(long)q * way + k];
    int n = 0;
    for (int s = 0; s < Ns; ++s) n += cls[s] == c;
    sg[c] = n ? -logits[(long)q * way + c] * (dlogits[(long)q * way + c] - dot) / (float)n : 0.f;
  }
  __syncthreads();
  for (int t0 = 0; t0 < 2 * Ns; t0 += blockDim.x) {
    const int t = t0 + threadIdx.x;
    const bool on = t < 2 * Ns;
    const int s = on ? t >> 1 : 0, dir = t & 1;
    const float* pb = dist + (long)q * L * ldd + (long)s * L;
    float* ob = dD + (long)q * L * ldd + (long)s * L;
    OtTab<LT> T;
    if constexpr (LT == 0) { T.base = ot_lds + threadIdx.x; T.stride = blockDim.x; T.L = L; }
    if (on) {
      const int c = cls[s];
      const float gs = c >= 0 && c < way ? sg[c] : 0.f;
      ot_fill<LT>(T, pb, dir ? 1 : ldd, dir ? ldd : 1, L);
      ot_back<LT>(T, pb, dir ? 1 : ldd, dir ? ldd : 1, L, gs);
    }
    // dD[r][c] of the block = E_A[r][c+1] + E_B[c][r+1]: the partner lane (t ^ 1) holds the other direction's table.  Own cell (l, k)
    // is block element (l, k) for direction A and (k, l) for direction B; each element is written once, even block rows by A, odd by B.
    if constexpr (LT == 0) {
      __syncthreads();
      if (on) {
        OtTab<0> O = T;
        O.base = ot_lds + (threadIdx.x ^ 1);
        for (int l = 0; l < L; ++l)
          for (int k = 0; k < L; ++k) {
            const int r = dir ? k : l, cc = dir ? l : k;
            if ((r & 1) == dir) ob[(long)r * ldd + cc] = T.C(l, k + 1) + O.C(k, l + 1);
          }
      }
      __syncthreads();
    } else if (on) {
#pragma unroll
      for (int l = 0; l < L; ++l)
#pragma unroll
        for (int k = 0; k < L; ++k) {
          const float v = T.C(l, k + 1) + __shfl_xor(T.C(k, l + 1), 1, 64);
          const int r = dir ? k : l, cc = dir ? l : k;
          if ((r & 1) == dir) ob[(long)r * ldd + cc] = v;
        }
    }
  }
}

static inline void ot_lds_attr(std::atomic<unsigned long long>& mask, const void* fn) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  const unsigned long long bit = 1ull << (d & 63);
  if (mask.load(std::memory_order_acquire) & bit) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, OT_LDS_BUDGET) == hipSuccess)
    mask.fetch_or(bit, std::memory_order_release);      // otherwise the launch that follows fails with its own message
}

// lanes of the workgroup: 2 Ns rounded up to a wavefront; the LDS path holds at most the lanes whose tables fit its budget
static int ot_block(int Ns, int L, bool reg) {
  int lanes = (2 * Ns + 63) & ~63;
  if (reg) return lanes;
  int fit = (int)(OT_LDS_BUDGET / (ot_cells(L) * sizeof(float))) & ~63;
  if (fit > 1024) fit = 1024;
  return lanes < fit ? lanes : fit;
}

static int ot_check_align(const char* who, int Nq, int Ns, int way, int L, const int* cls_host) {
  if (int rc = ot_check_dims(who, Nq, Ns, L, 4)) return rc;
  LMKD_REQUIRE(way >= 1 && way <= Ns, "%s: way %d outside 1 .. %d support videos", who, way, Ns);
  LMKD_REQUIRE(cls_host, "%s: the host copy of the support classes is missing", who);
  for (int s = 0; s < Ns; ++s) LMKD_REQUIRE(cls_host[s] >= 0 && cls_host[s] < way, "%s: support %d has class %d outside [0, %d)", who, s, cls_host[s], way);
  return LMKD_OK;
}

extern "C" int lmkd_otam_align_fwd(const float* dist, const int* sup_class, const int* sup_class_host, float* cum, float* logits, int Nq,
                                   int Ns, int way, int L, void* stream) {
  if (int rc = ot_check_align("lmkd_otam_align_fwd", Nq, Ns, way, L, sup_class_host)) return rc;
  LMKD_REQUIRE(dist && sup_class && cum && logits, "lmkd_otam_align_fwd: null pointer");
  const int ldd = (int)ot_ldd(Ns, L);
  const bool reg = L == OT_REG_L && 2 * Ns <= OT_REG_LANES;
  const int block = ot_block(Ns, L, reg);
  hipStream_t st = (hipStream_t)stream;
  if (reg) {
    hipLaunchKernelGGL(otam_align_fwd_kernel<OT_REG_L>, dim3(Nq), dim3(block), 0, st, dist, sup_class, cum, logits, Ns, way, L, ldd);
  } else {
    static std::atomic<unsigned long long> mask{0};
    ot_lds_attr(mask, reinterpret_cast<const void*>(otam_align_fwd_kernel<0>));
    hipLaunchKernelGGL(otam_align_fwd_kernel<0>, dim3(Nq), dim3(block), (size_t)ot_cells(L) * block * sizeof(float), st, dist, sup_class, cum,
                       logits, Ns, way, L, ldd);
  }
  LMKD_CHECK_LAUNCH("lmkd_otam_align_fwd");
  return LMKD_OK;
}

extern "C" int lmkd_otam_align_bwd(const float* dlogits, const float* logits, const float* dist, const int* sup_class,
                                   const int* sup_class_host, float* dD, int Nq, int Ns, int way, int L, void* stream) {
  if (int rc = ot_check_align("lmkd_otam_align_bwd", Nq, Ns, way, L, sup_class_host)) return rc;
  LMKD_REQUIRE(dlogits && logits && dist && sup_class && dD, "lmkd_otam_align_bwd: null pointer");
  const int ldd = (int)ot_ldd(Ns, L);
  const bool reg = L == OT_REG_L && 2 * Ns <= OT_REG_LANES;
  const int block = ot_block(Ns, L, reg);
  hipStream_t st = (hipStream_t)stream;
  if (reg) {
    hipLaunchKernelGGL(otam_align_bwd_kernel<OT_REG_L>, dim3(Nq), dim3(block), 0, st, dist, sup_class, logits, dlogits, dD, Ns, way, L, ldd);
  } else {
    static std::atomic<unsigned long long> mask{0};
    ot_lds_attr(mask, reinterpret_cast<const void*>(otam_align_bwd_kernel<0>));
    hipLaunchKernelGGL(otam_align_bwd_kernel<0>, dim3(Nq), dim3(block), (size_t)ot_cells(L) * block * sizeof(float), st, dist, sup_class, logits,
                       dlogits, dD, Ns, way, L, ldd);
  }
  LMKD_CHECK_LAUNCH("lmkd_otam_align_bwd");
  return LMKD_OK;
}
