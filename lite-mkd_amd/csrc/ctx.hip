// CTX matcher head (reference: teacher/code/model.py:2840-2936 CrossTransformer, the head of CTXBranch / TwoCTXShuffleTime): the
// frame-level cross-transformer - DESIGN.md 18.  K [(Ns + Nq) L][D] normalised keys, V the raw values, support videos first.  The
// classes are segments of the class-sorted support positions: position p holds video order[p], segment s the positions
// off[s] .. off[s] + cnt[s] - 1, F = cnt[s] L frames.  For query q and segment s
//   A = softmax_rows(Kq Kc^T / sqrt(D))   [L][F], evaluated after the row maximum is subtracted
//   logits[q][col[s]] = -|Vq - A Vc|_F^2 / L
// The prototypes A Vc are never stored: forward and backward form them column by column in registers; the backward keeps
// E = d loss / d (Vq - A Vc) between its two launches.  A (and the backward's dS) are [Nq L][Ns L] with column p L + frame.  Every sum
// runs in a fixed order: no atomics, two calls are bit-identical.
#include "rows.h"
#include <atomic>

#define LMKD_MAX_SEG 16
#define CX_MAX_L 16
#define CX_MAX_FRAMES 256          // support frames of one class (32 shots of 8 frames): the LDS plan of ctx_bwd_scores_kernel, DESIGN.md 18
#define CX_THREADS 256
#define CX_BIG 1024                // lanes of the per-(query, class) workgroups: 16 waves hide the latency of their small loops
#define CX_DTILE CX_BIG            // columns of D whose distance gradient ctx_bwd_scores_kernel holds in LDS at a time (one per lane)
#define CX_COLS 64                 // columns of D per workgroup of ctx_bwd_rows_kernel (one per lane, four waves split the sums)
#define CX_PF 8                    // loads a lane requests before it uses the first
#define CX_COEF 4096               // floats of attention coefficients ctx_bwd_rows_kernel stages at a time: 16 x 256 = 2 x 8 x 16 x 16
#define CX_LDS_BUDGET (128 * 1024)

struct CxSegs {
  int n;
  int off[LMKD_MAX_SEG];   // first class-sorted support position
  int cnt[LMKD_MAX_SEG];   // support videos
  int col[LMKD_MAX_SEG];   // logit column (the class label)
};

// LayerNorm over the rows of Kraw that keeps what lmkd_layernorm_bwd_rows reads (Khat and rstd, nullable); Kn may be Kraw itself.  The
// instance of csrc/rows.h that re-reads the row from global memory: no LDS limit on D
extern "C" int lmkd_ctx_ln_fwd(const float* Kraw, const float* gamma, const float* beta, float* Kn, float* Khat, float* rstd, long rows,
                               int D, float eps, void* stream) {
  LMKD_REQUIRE(rows >= 1 && rows < (1L << 31) && D >= 1, "lmkd_ctx_ln_fwd: %ld rows of %d", rows, D);
  LMKD_REQUIRE(Kraw && gamma && beta && Kn, "lmkd_ctx_ln_fwd: null pointer");
  hipLaunchKernelGGL((ln_fwd_kernel<false, true>), dim3((unsigned)rows), dim3(ROW_THREADS), 0, (hipStream_t)stream, Kraw, (const float*)nullptr, 0L,
                     gamma, beta, (const float*)nullptr, Kn, (long)D, Khat, rstd, D, eps);
  LMKD_CHECK_LAUNCH("lmkd_ctx_ln_fwd");
  return LMKD_OK;
}

// row of K / V that holds frame f of segment positions p0 ..: -1 when the order table names no support video (the lane then adds 0)
__device__ __forceinline__ int cx_row(const int* __restrict__ order, int p0, int f, int L, int Ns) {
  const int v = order[p0 + f / L];
  return v >= 0 && v < Ns ? v * L + f % L : -1;
}

// sum over a workgroup of CX_BIG lanes, the waves' sums added in wave order; valid in every lane
__device__ __forceinline__ float cx_block_sum(float v, float* red /* CX_BIG / 64 floats */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float a = 0.f;
  for (int w = 0; w < CX_BIG / 64; ++w) a += red[w];
  return a;
}

// pr[l] = sum_f A[l F + f] X[rows[f]][d] for one column d: CX_PF rows are requested before the first is used, so the lane keeps CX_PF loads
// in flight (the loop is latency bound: F independent 4-byte loads per column)
__device__ __forceinline__ void cx_proto_col(float (&pr)[CX_MAX_L], const float* __restrict__ A, const int* __restrict__ rows,
                                             const float* __restrict__ X, int F, int L, int D, int d) {
#pragma unroll
  for (int l = 0; l < CX_MAX_L; ++l) pr[l] = 0.f;
  for (int f0 = 0; f0 < F; f0 += CX_PF) {
    float vv[CX_PF];
#pragma unroll
    for (int j = 0; j < CX_PF; ++j) {
      const int r = f0 + j < F ? rows[f0 + j] : -1;
      vv[j] = r >= 0 ? X[(long)r * D + d] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < CX_PF; ++j)
      if (f0 + j < F) {
#pragma unroll
        for (int l = 0; l < CX_MAX_L; ++l)
          if (l < L) pr[l] += A[l * F + f0 + j] * vv[j];
      }
  }
}

// One workgroup of CX_BIG lanes per (query, segment).  Dynamic LDS: A [L][F] | rows [F] | key tile [L][CX_DTILE].
__global__ __launch_bounds__(CX_BIG) void ctx_attend_fwd_kernel(const float* __restrict__ K, const float* __restrict__ V,
                                                                const int* __restrict__ order, float* __restrict__ Ag,
                                                                float* __restrict__ logits, int Ns, int way, int L, int D, int Fmax,
                                                                CxSegs sg) {
  extern __shared__ float cx_lds[];
  __shared__ float red[CX_BIG / 64];
  const int q = blockIdx.x, s = blockIdx.y, p0 = sg.off[s], F = sg.cnt[s] * L;
  float* A = cx_lds;
  int* rows = (int*)(cx_lds + (long)L * Fmax);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long ldA = (long)Ns * L;
  const float* Kq = K + (long)(Ns + q) * L * D;
  const float* Vq = V + (long)(Ns + q) * L * D;
  // classes without a support video: their column is 0 (the reference's torch.zeros)
  if (s == 0)
    for (int c = threadIdx.x; c < way; c += CX_BIG) {
      bool has = false;
      for (int i = 0; i < sg.n; ++i) has |= sg.col[i] == c;
      if (!has) logits[(long)q * way + c] = 0.f;
    }
  for (int f = threadIdx.x; f < F; f += CX_BIG) rows[f] = cx_row(order, p0, f, L, Ns);
  __syncthreads();
  const float sc = 1.f / sqrtf((float)D);
  // scores, CX_DTILE columns of D at a time: the query's key rows of the tile go to LDS, then one wave per support frame with the lanes
  // along D adds the tile's share to A (frame f belongs to one wave: its cells have one writer)
  float* Kt = (float*)(rows + Fmax);
  for (int i = threadIdx.x; i < L * F; i += CX_BIG) A[i] = 0.f;
  for (int t0 = 0; t0 < D; t0 += CX_DTILE) {
    const int nd = D - t0 < CX_DTILE ? D - t0 : CX_DTILE;
    __syncthreads();
#pragma unroll
    for (int l = 0; l < CX_MAX_L; ++l)
      if (l < L) Kt[l * CX_DTILE + threadIdx.x] = (int)threadIdx.x < nd ? Kq[(long)l * D + t0 + threadIdx.x] : 0.f;
    __syncthreads();
    for (int f = wave; f < F; f += CX_BIG / 64) {
      const int r = rows[f];
      if (r < 0) continue;
      float kv[CX_DTILE / 64], acc[CX_MAX_L];
#pragma unroll
      for (int j = 0; j < CX_DTILE / 64; ++j) kv[j] = lane + 64 * j < nd ? K[(long)r * D + t0 + lane + 64 * j] : 0.f;
#pragma unroll
      for (int l = 0; l < CX_MAX_L; ++l) acc[l] = 0.f;
#pragma unroll
      for (int j = 0; j < CX_DTILE / 64; ++j) {
#pragma unroll
        for (int l = 0; l < CX_MAX_L; ++l)
          if (l < L) acc[l] += Kt[l * CX_DTILE + lane + 64 * j] * kv[j];
      }
#pragma unroll
      for (int l = 0; l < CX_MAX_L; ++l)
        if (l < L) {
          const float a = wave_sum(acc[l]);
          if (lane == 0) A[l * F + f] += a * sc;
        }
    }
  }
  __syncthreads();
  for (int l = wave; l < L; l += CX_BIG / 64) {      // softmax: one wave per query frame
    float m = -INFINITY;
    for (int f = lane; f < F; f += 64) m = fmaxf(m, A[l * F + f]);
    m = wave_max(m);
    float sum = 0.f;
    for (int f = lane; f < F; f += 64) {
      const float e = expf(A[l * F + f] - m);
      A[l * F + f] = e;
      sum += e;
    }
    const float inv = 1.f / wave_sum(sum);
    for (int f = lane; f < F; f += 64) {
      const float a = A[l * F + f] * inv;
      A[l * F + f] = a;
      if (Ag) Ag[((long)q * L + l) * ldA + (long)p0 * L + f] = a;
    }
  }
  __syncthreads();
  float dist = 0.f;
  for (int d = threadIdx.x; d < D; d += CX_BIG) {      // distance: one lane per column of D
    float pr[CX_MAX_L];
    cx_proto_col(pr, A, rows, V, F, L, D, d);
#pragma unroll
    for (int l = 0; l < CX_MAX_L; ++l)
      if (l < L) {
        const float df = Vq[(long)l * D + d] - pr[l];
        dist += df * df;
      }
  }
  dist = cx_block_sum(dist, red);
  if (threadIdx.x == 0) logits[(long)q * way + sg.col[s]] = -dist / (float)L;
}

// Backward, launch 1 of 2: one workgroup of CX_BIG lanes per (query, segment).  E = d loss / d (Vq - A Vc) = -2 g / L (Vq - A Vc) is
// formed CX_DTILE columns at a time (one per lane) and written to Eg [nseg][Nq L][D];  dA = -E Vc^T;  dS = A (dA - sum_f A dA) / sqrt(D),
// laid out like A.  Dynamic LDS: A [L][F] | dA [L][F] | E tile [L][CX_DTILE] | rows [F].
__global__ __launch_bounds__(CX_BIG) void ctx_bwd_scores_kernel(const float* __restrict__ g, const float* __restrict__ V,
                                                                const int* __restrict__ order, const float* __restrict__ Ag,
                                                                float* __restrict__ dSg, float* __restrict__ Eg, int Ns, int Nq, int way,
                                                                int L, int D, int Fmax, CxSegs sg) {
  extern __shared__ float cx_lds[];
  const int q = blockIdx.x, s = blockIdx.y, p0 = sg.off[s], F = sg.cnt[s] * L;
  float* A = cx_lds;
  float* dA = A + (long)L * Fmax;
  float* Et = dA + (long)L * Fmax;
  int* rows = (int*)(Et + (long)L * CX_DTILE);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long ldA = (long)Ns * L;
  const float* Vq = V + (long)(Ns + q) * L * D;
  float* Eo = Eg + ((long)s * Nq + q) * L * D;
  const float cf = -2.f * g[(long)q * way + sg.col[s]] / (float)L;
  for (int f = threadIdx.x; f < F; f += CX_BIG) rows[f] = cx_row(order, p0, f, L, Ns);
  for (int i = threadIdx.x; i < L * F; i += CX_BIG) {
    A[i] = Ag[((long)q * L + i / F) * ldA + (long)p0 * L + i % F];
    dA[i] = 0.f;
  }
  __syncthreads();
  for (int t0 = 0; t0 < D; t0 += CX_DTILE) {
    {
      const int dd = threadIdx.x, d = t0 + dd;      // CX_DTILE == CX_BIG: one column per lane
      float pr[CX_MAX_L];
      if (d < D) cx_proto_col(pr, A, rows, V, F, L, D, d);
#pragma unroll
      for (int l = 0; l < CX_MAX_L; ++l)
        if (l < L) {
          const float e = d < D ? cf * (Vq[(long)l * D + d] - pr[l]) : 0.f;
          Et[l * CX_DTILE + dd] = e;
          if (d < D) Eo[(long)l * D + d] = e;
        }
    }
    __syncthreads();
    const int nd = D - t0 < CX_DTILE ? D - t0 : CX_DTILE;
    for (int f = wave; f < F; f += CX_BIG / 64) {      // frame f belongs to this wave alone in every tile: its dA cells have one writer
      const int r = rows[f];
      if (r < 0) continue;
      float vv[CX_DTILE / 64], acc[CX_MAX_L];
#pragma unroll
      for (int j = 0; j < CX_DTILE / 64; ++j) vv[j] = lane + 64 * j < nd ? V[(long)r * D + t0 + lane + 64 * j] : 0.f;
#pragma unroll
      for (int l = 0; l < CX_MAX_L; ++l) acc[l] = 0.f;
#pragma unroll
      for (int j = 0; j < CX_DTILE / 64; ++j) {      // (columns past D hold 0 in the tile)
#pragma unroll
        for (int l = 0; l < CX_MAX_L; ++l)
          if (l < L) acc[l] += Et[l * CX_DTILE + lane + 64 * j] * vv[j];
      }
#pragma unroll
      for (int l = 0; l < CX_MAX_L; ++l)
        if (l < L) {
          const float a = wave_sum(acc[l]);
          if (lane == 0) dA[l * F + f] -= a;
        }
    }
    __syncthreads();
  }
  const float sc = 1.f / sqrtf((float)D);
  for (int l = wave; l < L; l += CX_BIG / 64) {
    float dot = 0.f;
    for (int f = lane; f < F; f += 64) dot += A[l * F + f] * dA[l * F + f];
    dot = wave_sum(dot);
    for (int f = lane; f < F; f += 64)
      dSg[((long)q * L + l) * ldA + (long)p0 * L + f] = A[l * F + f] * (dA[l * F + f] - dot) * sc;
  }
}

// Backward, launch 2 of 2: one workgroup of 4 waves per (video, CX_COLS columns of D), one lane per column; given A, dS and E every row
// gradient is independent along D.  The waves split the sum (wave w takes the queries / the support frames w, w + 4, ..) and their partial
// sums are added in wave order.  Blocks 0 .. Ns-1: the support video at class-sorted position blockIdx.x,
//   dVc[m] = -sum_q sum_l A_q[l][m] E_q[l],  dKc[m] = sum_q sum_l dS_q[l][m] Kq[l];
// blocks Ns ..: query blockIdx.x - Ns,  dVq[l] = sum_s E_s[l],  dKq[l] = sum_s sum_f dS[l][f] Kc[f].
// Static LDS: cf [CX_COEF] coefficients (A and dS of the video's frames for a chunk of queries; dS of a segment) | part: the waves' sums.
__global__ __launch_bounds__(CX_THREADS) void ctx_bwd_rows_kernel(const float* __restrict__ K, const int* __restrict__ order,
                                                                  const float* __restrict__ Ag, const float* __restrict__ dSg,
                                                                  const float* __restrict__ Eg, float* __restrict__ dK,
                                                                  float* __restrict__ dV, int Ns, int Nq, int L, int D, CxSegs sg) {
  __shared__ float cfs[CX_COEF];
  __shared__ int rows[CX_MAX_FRAMES];
  __shared__ float part[4][2][CX_MAX_L][CX_COLS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = blockIdx.y * CX_COLS + lane;
  const bool on = d < D;
  const long ldA = (long)Ns * L;
  float dv[CX_MAX_L], dk[CX_MAX_L];
#pragma unroll
  for (int l = 0; l < CX_MAX_L; ++l) dv[l] = dk[l] = 0.f;
  long orow;
  if ((int)blockIdx.x >= Ns) {
    const int q = blockIdx.x - Ns;
    orow = (long)(Ns + q) * L;
    for (int s = 0; s < sg.n; ++s) {
      const int p0 = sg.off[s], F = sg.cnt[s] * L;
      __syncthreads();
      for (int f = threadIdx.x; f < F; f += CX_THREADS) rows[f] = cx_row(order, p0, f, L, Ns);
      for (int i = threadIdx.x; i < L * F; i += CX_THREADS) cfs[i] = dSg[((long)q * L + i / F) * ldA + (long)p0 * L + i % F];
      __syncthreads();
      if (!on) continue;
      if ((s & 3) == wave) {
        const float* Eo = Eg + ((long)s * Nq + q) * L * D;
#pragma unroll
        for (int l = 0; l < CX_MAX_L; ++l)
          if (l < L) dv[l] += Eo[(long)l * D + d];
      }
      for (int f0 = wave; f0 < F; f0 += 4 * CX_PF) {
        float kk[CX_PF];
#pragma unroll
        for (int j = 0; j < CX_PF; ++j) {
          const int f = f0 + 4 * j, r = f < F ? rows[f] : -1;
          kk[j] = r >= 0 ? K[(long)r * D + d] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < CX_PF; ++j) {
          const int f = f0 + 4 * j;
          if (f < F) {
#pragma unroll
            for (int l = 0; l < CX_MAX_L; ++l)
              if (l < L) dk[l] += cfs[l * F + f] * kk[j];
          }
        }
      }
    }
  } else {
    const int p = blockIdx.x;
    int s = 0;
    while (s < sg.n - 1 && p >= sg.off[s] + sg.cnt[s]) ++s;
    const int v = order[p];
    if (v < 0 || v >= Ns) return;      // the whole workgroup: nothing to own
    orow = (long)v * L;
    const int LL = L * L, QC = (CX_COEF / 2) / LL;      // queries per chunk of coefficients: cfs = A part [QC][L][L] | dS part [QC][L][L]
    for (int q0 = 0; q0 < Nq; q0 += QC) {
      const int nq = Nq - q0 < QC ? Nq - q0 : QC;
      __syncthreads();
      for (int i = threadIdx.x; i < nq * LL; i += CX_THREADS) {
        const int qi = i / LL, l = (i % LL) / L, m = i % L;
        const long at = ((long)(q0 + qi) * L + l) * ldA + (long)p * L + m;
        cfs[i] = Ag[at];
        cfs[QC * LL + i] = dSg[at];
      }
      __syncthreads();
      if (!on) continue;
      for (int qi = wave; qi < nq; qi += 4) {
        const int q = q0 + qi;
        const float* Eo = Eg + ((long)s * Nq + q) * L * D;
        const float* Kq = K + (long)(Ns + q) * L * D;
        float e[CX_MAX_L], kq[CX_MAX_L];
#pragma unroll
        for (int l = 0; l < CX_MAX_L; ++l)
          if (l < L) { e[l] = Eo[(long)l * D + d]; kq[l] = Kq[(long)l * D + d]; }
#pragma unroll
        for (int l = 0; l < CX_MAX_L; ++l)
          if (l < L) {
            const float* a = cfs + qi * LL + l * L;
            const float* ds = a + QC * LL;
#pragma unroll
            for (int m = 0; m < CX_MAX_L; ++m)
              if (m < L) {
                dv[m] -= a[m] * e[l];
                dk[m] += ds[m] * kq[l];
              }
          }
      }
    }
  }
#pragma unroll
  for (int l = 0; l < CX_MAX_L; ++l)
    if (l < L) {
      part[wave][0][l][lane] = dv[l];
      part[wave][1][l][lane] = dk[l];
    }
  __syncthreads();
  if (!on) return;
  for (int l = wave; l < L; l += 4) {
    dV[(orow + l) * D + d] = ((part[0][0][l][lane] + part[1][0][l][lane]) + part[2][0][l][lane]) + part[3][0][l][lane];
    dK[(orow + l) * D + d] = ((part[0][1][l][lane] + part[1][1][l][lane]) + part[2][1][l][lane]) + part[3][1][l][lane];
  }
}

// every shape check of the attend entry points; fills the kernel's copy of the class layout and the largest frame count of a class
static int cx_check(const char* who, int Ns, int Nq, int way, int L, int D, int nseg, const int* seg_off, const int* seg_cnt,
                    const int* seg_col, CxSegs* sg, int* Fmax) {
  LMKD_REQUIRE(L >= 1 && L <= CX_MAX_L, "%s: seq_len %d outside 1 .. %d", who, L, CX_MAX_L);
  LMKD_REQUIRE(D >= 4 && D % 4 == 0, "%s: D = %d is not a positive multiple of 4", who, D);
  LMKD_REQUIRE(Ns >= 1 && Nq >= 1 && way >= 1, "%s: %d support videos, %d queries, way %d", who, Ns, Nq, way);
  LMKD_REQUIRE((long)Nq * L * Ns * L < (1L << 31) && (long)(Ns + Nq) * L * D < (1L << 40), "%s: %d x %d videos of %d frames", who, Ns, Nq, L);
  LMKD_REQUIRE(nseg >= 1 && nseg <= LMKD_MAX_SEG, "%s: %d classes with support outside 1 .. %d", who, nseg, LMKD_MAX_SEG);
  LMKD_REQUIRE(seg_off && seg_cnt && seg_col, "%s: the host class layout is missing", who);
  memset(sg, 0, sizeof(*sg));
  sg->n = nseg;
  int at = 0, fm = 0;
  for (int i = 0; i < nseg; ++i) {
    LMKD_REQUIRE(seg_col[i] >= 0 && seg_col[i] < way, "%s: class column %d outside [0, %d)", who, seg_col[i], way);
    LMKD_REQUIRE(seg_cnt[i] >= 1 && seg_off[i] == at, "%s: segment %d (offset %d, %d videos) does not follow position %d", who, i, seg_off[i],
                 seg_cnt[i], at);
    LMKD_REQUIRE((long)seg_cnt[i] * L <= CX_MAX_FRAMES, "%s: %ld support frames in class %d, at most %d", who, (long)seg_cnt[i] * L, seg_col[i],
                 CX_MAX_FRAMES);
    sg->off[i] = seg_off[i]; sg->cnt[i] = seg_cnt[i]; sg->col[i] = seg_col[i];
    at += seg_cnt[i];
    if (seg_cnt[i] * L > fm) fm = seg_cnt[i] * L;
  }
  LMKD_REQUIRE(at == Ns, "%s: the segments hold %d support videos, not %d", who, at, Ns);
  *Fmax = fm;
  return LMKD_OK;
}

static inline void cx_lds_attr(std::atomic<unsigned long long>& mask, const void* fn) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  const unsigned long long bit = 1ull << (d & 63);
  if (mask.load(std::memory_order_acquire) & bit) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, CX_LDS_BUDGET) == hipSuccess)
    mask.fetch_or(bit, std::memory_order_release);      // otherwise the launch that follows fails with its own message
}

extern "C" int lmkd_ctx_attend_fwd(const float* K, const float* V, const int* order, float* A, float* logits, int Ns, int Nq, int way, int L,
                                   int D, int nseg, const int* seg_off, const int* seg_cnt, const int* seg_col, void* stream) {
  CxSegs sg;
  int Fmax = 0;
  if (int rc = cx_check("lmkd_ctx_attend_fwd", Ns, Nq, way, L, D, nseg, seg_off, seg_cnt, seg_col, &sg, &Fmax)) return rc;
  LMKD_REQUIRE(K && V && order && logits, "lmkd_ctx_attend_fwd: null pointer");
  const size_t lds = ((size_t)L * Fmax + Fmax + (size_t)L * CX_DTILE) * sizeof(float);      // at most 81 KB: L 16, 256 frames
  static std::atomic<unsigned long long> mask{0};
  cx_lds_attr(mask, reinterpret_cast<const void*>(ctx_attend_fwd_kernel));
  hipLaunchKernelGGL(ctx_attend_fwd_kernel, dim3(Nq, nseg), dim3(CX_BIG), lds, (hipStream_t)stream, K, V, order, A, logits, Ns, way, L, D,
                     Fmax, sg);
  LMKD_CHECK_LAUNCH("lmkd_ctx_attend_fwd");
  return LMKD_OK;
}

extern "C" int lmkd_ctx_attend_bwd(const float* dlogits, const float* K, const float* V, const int* order, const float* A, float* dS,
                                   float* E, float* dK, float* dV, int Ns, int Nq, int way, int L, int D, int nseg, const int* seg_off,
                                   const int* seg_cnt, const int* seg_col, void* stream) {
  CxSegs sg;
  int Fmax = 0;
  if (int rc = cx_check("lmkd_ctx_attend_bwd", Ns, Nq, way, L, D, nseg, seg_off, seg_cnt, seg_col, &sg, &Fmax)) return rc;
  LMKD_REQUIRE(dlogits && K && V && order && A && dS && E && dK && dV, "lmkd_ctx_attend_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds1 = ((size_t)2 * L * Fmax + (size_t)L * CX_DTILE + Fmax) * sizeof(float);      // at most 98 KB: L 16, 256 frames
  static std::atomic<unsigned long long> mask{0};
  cx_lds_attr(mask, reinterpret_cast<const void*>(ctx_bwd_scores_kernel));
  hipLaunchKernelGGL(ctx_bwd_scores_kernel, dim3(Nq, nseg), dim3(CX_BIG), lds1, st, dlogits, V, order, A, dS, E, Ns, Nq, way, L, D, Fmax, sg);
  LMKD_CHECK_LAUNCH("lmkd_ctx_attend_bwd (scores)");
  hipLaunchKernelGGL(ctx_bwd_rows_kernel, dim3(Ns + Nq, cdiv(D, CX_COLS)), dim3(CX_THREADS), 0, st, K, order, A, (const float*)dS,
                     (const float*)E, dK, dV, Ns, Nq, L, D, sg);
  LMKD_CHECK_LAUNCH("lmkd_ctx_attend_bwd (rows)");
  return LMKD_OK;
}
