// STRM student family (model/backbone/strm18_student.py, strmbackbone.py; model/classifiers/strm_res18_sup.py): the small operators
// between the ResNet-18 trunk and the TRX heads that have no kernel elsewhere in the library.
//
//   patch pooling    AdaptiveMaxPool2d((4,4)) with the 16 patches KEPT, the positional table and the dropout mask of Self_Attn_Bot.pe
//                    applied in the same launch, and the arg-max byte per output; backward is a gather over the windows of a pixel
//   patch attention  per frame: energy = Q K^T (unscaled, 16 x 16 dot products of C terms), row softmax, out = attn V, y = gamma out + x;
//                    backward gives dQ | dK | dV in one [F,16,3C] block and one dgamma partial per frame
//   token MLP        per video and channel over the L frames (2 <= L <= 16): y = W2 relu(W1 xp + b1) + b2 + xp with xp = (x + pe) * mask
//   patch distance   DistanceLoss: relu(P_a[i] + P_b[j] + b) per frame pair, the minimum Euclidean distance of every query pair row to the
//                    pair rows of each class in the difference form sum (q - s)^2, the arg-min, the mean over the pairs, negated
//
// All tensors fp32, fp32 accumulation.  Every reduction has a fixed order (lane partials -> xor butterflies / LDS trees -> per-workgroup
// partial rows -> strm_reduce_rows_k), so results are run-to-run bit-identical; no float atomics.  These are latency-bound kernels on
// small tensors: one launch per operator and direction, nothing staged through HBM that a launch can keep.
#include "common.h"

#define ST_THREADS 256
#define ST_NP 16           // patches per frame (4 x 4)
#define ST_KC 256          // columns of Q / K staged in LDS per step of the energy products
#define ST_LD (ST_KC + 4)  // row stride of the staged tiles: consecutive rows start 4 banks apart, so 16 rows read 16 distinct 16-byte slots
#define ST_L 8             // frames per video of the token MLP's own kernels (args.seq_len of every configuration of the reference)
#define ST_LMAX 16         // longest clip of the templated token-MLP family and of the patch-distance head
#define ST_TOK 144         // token-MLP parameter gradients: dW1 [8][8] | db1 [8] | dW2 [8][8] | db2 [8]
#define ST_HD 1024         // width of DistanceLoss.clsW's output
#define ST_QR 4            // query pair rows per wave of the minimum-distance kernels
#define ST_SB 8            // support pair rows per LDS block of the tiled minimum-distance kernel (4 KB each)

static inline int st_grid(long n) { return (int)((n + ST_THREADS - 1) / ST_THREADS); }
__device__ __forceinline__ float4 sld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void sst4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

// ------------------------------------------------------------------------------------------------------------------------------------
// patch pooling
// ------------------------------------------------------------------------------------------------------------------------------------
// torch's adaptive windows: [floor(i n / 4), ceil((i + 1) n / 4))
__device__ __forceinline__ int win_lo(int i, int n) { return (i * n) / 4; }
__device__ __forceinline__ int win_hi(int i, int n) { return ((i + 1) * n + 3) / 4; }

__device__ __forceinline__ void pool_take(float v, int at, float& best, int& bi) {
  if (v > best || v != v) {      // aten: first maximum in row-major window order, NaN wins
    best = v;
    bi = at;
  }
}

__global__ void strm_patchpool_fwd_k(const float* __restrict__ x, const float* __restrict__ pe, const float* __restrict__ mask,
                                     float* __restrict__ y, unsigned char* __restrict__ idx, long F, int H, int W, int C) {
  const int C4 = C >> 2;
  const long t = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= F * ST_NP * C4) return;
  const int c = (int)(t % C4) * 4, p = (int)((t / C4) % ST_NP);
  const long f = t / ((long)C4 * ST_NP);
  const int h0 = win_lo(p >> 2, H), h1 = win_hi(p >> 2, H), w0 = win_lo(p & 3, W), w1 = win_hi(p & 3, W);
  const float* xf = x + f * H * W * C + c;
  float4 b = sld4(xf + ((long)h0 * W + w0) * C);
  int i0 = h0 * W + w0, i1 = i0, i2 = i0, i3 = i0;
  for (int h = h0; h < h1; ++h)
    for (int w = w0; w < w1; ++w) {
      const int at = h * W + w;
      const float4 v = sld4(xf + (long)at * C);
      pool_take(v.x, at, b.x, i0);
      pool_take(v.y, at, b.y, i1);
      pool_take(v.z, at, b.z, i2);
      pool_take(v.w, at, b.w, i3);
    }
  const float4 e = sld4(pe + p * C + c);
  float4 o = make_float4(b.x + e.x, b.y + e.y, b.z + e.z, b.w + e.w);
  const long at = (f * ST_NP + p) * C + c;
  if (mask) {
    const float4 m = sld4(mask + at);
    o = make_float4(o.x * m.x, o.y * m.y, o.z * m.z, o.w * m.w);
  }
  sst4(y + at, o);
  *reinterpret_cast<uchar4*>(idx + at) = make_uchar4((unsigned char)i0, (unsigned char)i1, (unsigned char)i2, (unsigned char)i3);
}

// dx[f,h,w,c] = sum over the (at most four) windows that hold (h,w) of dy * mask where the window's arg-max is (h,w): a gather
__global__ void strm_patchpool_bwd_k(const float* __restrict__ dy, const float* __restrict__ mask, const unsigned char* __restrict__ idx,
                                     float* __restrict__ dx, long F, int H, int W, int C) {
  const int C4 = C >> 2;
  const long t = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= F * H * W * C4) return;
  const int c = (int)(t % C4) * 4, at = (int)((t / C4) % (H * W));
  const long f = t / ((long)C4 * H * W);
  const int h = at / W, w = at % W;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ph = 0; ph < 4; ++ph) {
    if (h < win_lo(ph, H) || h >= win_hi(ph, H)) continue;
    for (int pw = 0; pw < 4; ++pw) {
      if (w < win_lo(pw, W) || w >= win_hi(pw, W)) continue;
      const long o = (f * ST_NP + ph * 4 + pw) * C + c;
      const uchar4 i = *reinterpret_cast<const uchar4*>(idx + o);
      float4 d = sld4(dy + o);
      if (mask) {
        const float4 m = sld4(mask + o);
        d = make_float4(d.x * m.x, d.y * m.y, d.z * m.z, d.w * m.w);
      }
      if (i.x == at) g.x += d.x;
      if (i.y == at) g.y += d.y;
      if (i.z == at) g.z += d.z;
      if (i.w == at) g.w += d.w;
    }
  }
  sst4(dx + (f * H * W + at) * C + c, g);
}

extern "C" int lmkd_strm_patchpool_fwd(const float* x, const float* pe, const float* mask, float* y, unsigned char* idx, int F, int H, int W,
                                       int C, void* stream) {
  LMKD_REQUIRE(x && pe && y && idx && F > 0 && H >= 1 && W >= 1 && H * W <= 256 && C > 0 && C % 4 == 0,
               "lmkd_strm_patchpool_fwd: needs H * W <= 256 (arg-max bytes) and C %% 4 == 0, got %dx%dx%d", H, W, C);
  LMKD_REQUIRE(aligned16(x) && aligned16(pe) && aligned16(y) && aligned16(mask) && (((uintptr_t)idx) & 3) == 0, "lmkd_strm_patchpool_fwd: unaligned tensor");
  hipLaunchKernelGGL(strm_patchpool_fwd_k, dim3(st_grid((long)F * ST_NP * (C / 4))), dim3(ST_THREADS), 0, (hipStream_t)stream, x, pe, mask, y,
                     idx, (long)F, H, W, C);
  LMKD_CHECK_LAUNCH("strm_patchpool_fwd_k");
  return LMKD_OK;
}

extern "C" int lmkd_strm_patchpool_bwd(const float* dy, const float* mask, const unsigned char* idx, float* dx, int F, int H, int W, int C,
                                       void* stream) {
  LMKD_REQUIRE(dy && idx && dx && F > 0 && H >= 1 && W >= 1 && H * W <= 256 && C > 0 && C % 4 == 0, "lmkd_strm_patchpool_bwd: bad arguments");
  LMKD_REQUIRE(aligned16(dy) && aligned16(dx) && aligned16(mask) && (((uintptr_t)idx) & 3) == 0, "lmkd_strm_patchpool_bwd: unaligned tensor");
  hipLaunchKernelGGL(strm_patchpool_bwd_k, dim3(st_grid((long)F * H * W * (C / 4))), dim3(ST_THREADS), 0, (hipStream_t)stream, dy, mask, idx,
                     dx, (long)F, H, W, C);
  LMKD_CHECK_LAUNCH("strm_patchpool_bwd_k");
  return LMKD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// patch attention: one workgroup per frame, lane t owns entry (i, j) = (t / 16, t % 16) of the 16 x 16 tile
// ------------------------------------------------------------------------------------------------------------------------------------
// a[i] . b[j] over C columns for the lane's (i, j); a, b: 16 rows of lda / ldb floats in global memory, staged ST_KC columns at a time
__device__ __forceinline__ float tile_dot(const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb, int C,
                                          float (*As)[ST_LD], float (*Bs)[ST_LD]) {
  const int t = threadIdx.x, i = t >> 4, j = t & 15;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = 0; k0 < C; k0 += ST_KC) {
    for (int e = t; e < ST_NP * (ST_KC / 4); e += ST_THREADS) {
      const int r = e / (ST_KC / 4), c = (e % (ST_KC / 4)) * 4;
      sst4(&As[r][c], sld4(a + r * lda + k0 + c));
      sst4(&Bs[r][c], sld4(b + r * ldb + k0 + c));
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < ST_KC; k += 4) {
      const float4 u = sld4(&As[i][k]), v = sld4(&Bs[j][k]);
      acc.x = fmaf(u.x, v.x, acc.x);
      acc.y = fmaf(u.y, v.y, acc.y);
      acc.z = fmaf(u.z, v.z, acc.z);
      acc.w = fmaf(u.w, v.w, acc.w);
    }
    __syncthreads();
  }
  return (acc.x + acc.y) + (acc.z + acc.w);
}

__global__ __launch_bounds__(ST_THREADS) void strm_attn_fwd_k(const float* __restrict__ x, const float* __restrict__ qkv,
                                                               const float* __restrict__ gamma, float* __restrict__ y,
                                                               float* __restrict__ P, int C) {
  __shared__ __attribute__((aligned(16))) float As[ST_NP][ST_LD];
  __shared__ __attribute__((aligned(16))) float Bs[ST_NP][ST_LD];
  __shared__ float Ps[ST_NP][ST_NP + 1];
  const long f = blockIdx.x;
  const int t = threadIdx.x, i = t >> 4, j = t & 15;
  const long ld = 3L * C;
  const float* q = qkv + f * ST_NP * ld;
  const float e = tile_dot(q, ld, q + C, ld, C, As, Bs);
  float m = e;
  for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
  float p = expf(e - m), s = p;
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
  p = p / s;
  Ps[i][j] = p;
  P[f * (ST_NP * ST_NP) + t] = p;
  __syncthreads();
  const float g = gamma[0];
  const float* v = q + 2 * C;
  for (int c = t; c < C; c += ST_THREADS) {
    float vv[ST_NP];
#pragma unroll
    for (int r = 0; r < ST_NP; ++r) vv[r] = v[r * ld + c];
#pragma unroll
    for (int r = 0; r < ST_NP; ++r) {
      float o = 0.f;
#pragma unroll
      for (int k = 0; k < ST_NP; ++k) o = fmaf(Ps[r][k], vv[k], o);
      const long at = (f * ST_NP + r) * C + c;
      y[at] = fmaf(g, o, x[at]);
    }
  }
}

// dqkv [F,16,3C] = dQ | dK | dV, dgamma_part[f] = sum_ij P_ij (dy_i . V_j)  ( = sum dy * out )
__global__ __launch_bounds__(ST_THREADS) void strm_attn_bwd_k(const float* __restrict__ dy, const float* __restrict__ qkv,
                                                               const float* __restrict__ P, const float* __restrict__ gamma,
                                                               float* __restrict__ dqkv, float* __restrict__ dgamma_part, int C) {
  __shared__ __attribute__((aligned(16))) float As[ST_NP][ST_LD];
  __shared__ __attribute__((aligned(16))) float Bs[ST_NP][ST_LD];
  __shared__ float Ps[ST_NP][ST_NP + 1];
  __shared__ float Es[ST_NP][ST_NP + 1];
  __shared__ float red[ST_THREADS];
  const long f = blockIdx.x;
  const int t = threadIdx.x, i = t >> 4, j = t & 15;
  const long ld = 3L * C;
  const float* q = qkv + f * ST_NP * ld;
  const float* d = dy + f * ST_NP * C;
  const float raw = tile_dot(d, C, q + 2 * C, ld, C, As, Bs);      // dy_i . V_j
  const float p = P[f * (ST_NP * ST_NP) + t];
  red[t] = p * raw;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) dgamma_part[f] = red[0];
  const float g = gamma[0];
  const float dp = g * raw;      // d loss / d attn_ij
  float rd = dp * p;
  for (int o = 8; o > 0; o >>= 1) rd += __shfl_xor(rd, o, 16);
  Ps[i][j] = p;
  Es[i][j] = p * (dp - rd);      // d loss / d energy_ij
  __syncthreads();
  float* o_ = dqkv + f * ST_NP * ld;
  for (int c = t; c < C; c += ST_THREADS) {
    float dv[ST_NP], qv[ST_NP], kv[ST_NP];
#pragma unroll
    for (int r = 0; r < ST_NP; ++r) {
      dv[r] = d[r * C + c];
      qv[r] = q[r * ld + c];
      kv[r] = q[r * ld + C + c];
    }
#pragma unroll
    for (int r = 0; r < ST_NP; ++r) {
      float aq = 0.f, ak = 0.f, av = 0.f;
#pragma unroll
      for (int k = 0; k < ST_NP; ++k) {
        aq = fmaf(Es[r][k], kv[k], aq);      // dQ_r = sum_k dE_rk K_k
        ak = fmaf(Es[k][r], qv[k], ak);      // dK_r = sum_k dE_kr Q_k
        av = fmaf(Ps[k][r], dv[k], av);      // dV_r = gamma sum_k P_kr dy_k
      }
      o_[r * ld + c] = aq;
      o_[r * ld + C + c] = ak;
      o_[r * ld + 2 * C + c] = g * av;
    }
  }
}

// out[m] (+)= sum over the n rows of part[n][m]: one workgroup per column, lane partials over rows t, t + 256, ... then an LDS tree
__global__ __launch_bounds__(ST_THREADS) void strm_reduce_rows_k(const float* __restrict__ part, float* __restrict__ out, int n, int m) {
  __shared__ float red[ST_THREADS];
  const int t = threadIdx.x, col = blockIdx.x;
  float s = 0.f;
  for (int r = t; r < n; r += ST_THREADS) s += part[(long)r * m + col];
  red[t] = s;
  __syncthreads();
  for (int k = ST_THREADS / 2; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) out[col] = red[0];
}

static int attn_check(const char* who, const void* a, const void* b, const void* c, const void* d, const void* e, int F, int C) {
  LMKD_REQUIRE(a && b && c && d && e && F > 0 && C >= ST_KC && C % ST_KC == 0, "%s: needs C %% %d == 0 and non-null tensors (C = %d)", who, ST_KC, C);
  LMKD_REQUIRE(aligned16(a) && aligned16(b), "%s: unaligned tensor", who);
  return LMKD_OK;
}

extern "C" int lmkd_strm_attn_fwd(const float* x, const float* qkv, const float* gamma, float* y, float* probs, int F, int C, void* stream) {
  if (int rc = attn_check("lmkd_strm_attn_fwd", qkv, x, gamma, y, probs, F, C)) return rc;
  hipLaunchKernelGGL(strm_attn_fwd_k, dim3(F), dim3(ST_THREADS), 0, (hipStream_t)stream, x, qkv, gamma, y, probs, C);
  LMKD_CHECK_LAUNCH("strm_attn_fwd_k");
  return LMKD_OK;
}

extern "C" int lmkd_strm_attn_bwd(const float* dy, const float* qkv, const float* probs, const float* gamma, float* dqkv, float* dgamma_part,
                                  float* dgamma, int F, int C, void* stream) {
  if (int rc = attn_check("lmkd_strm_attn_bwd", qkv, dy, probs, gamma, dqkv, F, C)) return rc;
  LMKD_REQUIRE(dgamma_part && dgamma, "lmkd_strm_attn_bwd: null dgamma buffers");
  hipLaunchKernelGGL(strm_attn_bwd_k, dim3(F), dim3(ST_THREADS), 0, (hipStream_t)stream, dy, qkv, probs, gamma, dqkv, dgamma_part, C);
  LMKD_CHECK_LAUNCH("strm_attn_bwd_k");
  hipLaunchKernelGGL(strm_reduce_rows_k, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, dgamma_part, dgamma, F, 1);
  LMKD_CHECK_LAUNCH("strm_reduce_rows_k");
  return LMKD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// token MLP along the frame axis (MLP_Mix_Enrich: pe + dropout, Tok_MLP over the 8 frames, residual): one lane per (video, channel)
// ------------------------------------------------------------------------------------------------------------------------------------
struct TokW {
  float w1[ST_L][ST_L], b1[ST_L], w2[ST_L][ST_L], b2[ST_L];
};
__device__ __forceinline__ void tok_load(TokW* s, const float* w1, const float* b1, const float* w2, const float* b2) {
  const int t = threadIdx.x;
  if (t < ST_L * ST_L) {
    (&s->w1[0][0])[t] = w1[t];
    (&s->w2[0][0])[t] = w2[t];
  }
  if (t < ST_L) {
    s->b1[t] = b1[t];
    s->b2[t] = b2[t];
  }
  __syncthreads();
}

__global__ __launch_bounds__(ST_THREADS) void strm_tokmlp_fwd_k(const float* __restrict__ x, const float* __restrict__ pe,
                                                                 const float* __restrict__ mask, const float* __restrict__ w1,
                                                                 const float* __restrict__ b1, const float* __restrict__ w2,
                                                                 const float* __restrict__ b2, float* __restrict__ xp, float* __restrict__ y,
                                                                 unsigned char* __restrict__ hmask, long V, int D) {
  __shared__ TokW s;
  tok_load(&s, w1, b1, w2, b2);
  const long t = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= V * D) return;
  const long v = t / D;
  const int d = (int)(t % D);
  float a[ST_L], h[ST_L];
#pragma unroll
  for (int l = 0; l < ST_L; ++l) {
    const long at = (v * ST_L + l) * D + d;
    float u = x[at] + pe[l * D + d];
    if (mask) u *= mask[at];
    a[l] = u;
    xp[at] = u;
  }
#pragma unroll
  for (int k = 0; k < ST_L; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < ST_L; ++l) acc = fmaf(s.w1[k][l], a[l], acc);
    h[k] = fmaxf(acc + s.b1[k], 0.f);
    if (hmask) hmask[(v * ST_L + k) * D + d] = h[k] > 0.f;
  }
#pragma unroll
  for (int o = 0; o < ST_L; ++o) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < ST_L; ++k) acc = fmaf(s.w2[o][k], h[k], acc);
    y[(v * ST_L + o) * D + d] = (acc + s.b2[o]) + a[o];
  }
}

// dx and one row of parameter-gradient partials per workgroup: part[blockIdx.x][dW1 | db1 | dW2 | db2]
__global__ __launch_bounds__(ST_THREADS) void strm_tokmlp_bwd_k(const float* __restrict__ dy, const float* __restrict__ xp,
                                                                 const float* __restrict__ mask, const float* __restrict__ w1,
                                                                 const float* __restrict__ b1, const float* __restrict__ w2,
                                                                 float* __restrict__ dx, float* __restrict__ part, long V, int D) {
  __shared__ TokW s;
  __shared__ float st[4][ST_L][ST_THREADS];      // dy | h | masked dh | xp of every lane
  tok_load(&s, w1, b1, w2, b1);
  const int tid = threadIdx.x;
  const long t = (long)blockIdx.x * ST_THREADS + tid;
  const bool live = t < V * D;
  const long v = live ? t / D : 0;
  const int d = live ? (int)(t % D) : 0;
  float a[ST_L], h[ST_L], g[ST_L], dh[ST_L];
#pragma unroll
  for (int l = 0; l < ST_L; ++l) {
    const long at = (v * ST_L + l) * D + d;
    a[l] = live ? xp[at] : 0.f;
    g[l] = live ? dy[at] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < ST_L; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < ST_L; ++l) acc = fmaf(s.w1[k][l], a[l], acc);
    h[k] = live ? fmaxf(acc + s.b1[k], 0.f) : 0.f;
  }
#pragma unroll
  for (int k = 0; k < ST_L; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < ST_L; ++o) acc = fmaf(s.w2[o][k], g[o], acc);
    dh[k] = h[k] > 0.f ? acc : 0.f;
  }
#pragma unroll
  for (int l = 0; l < ST_L; ++l) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < ST_L; ++k) acc = fmaf(s.w1[k][l], dh[k], acc);
    if (live) {
      const long at = (v * ST_L + l) * D + d;
      float r = g[l] + acc;
      if (mask) r *= mask[at];
      dx[at] = r;
    }
    st[0][l][tid] = g[l];
    st[1][l][tid] = h[l];
    st[2][l][tid] = dh[l];
    st[3][l][tid] = a[l];
  }
  __syncthreads();
  if (tid < ST_TOK) {
    const float *u, *w = nullptr;
    if (tid < 64) {      // dW1[k][l] = sum dh_k xp_l
      u = st[2][tid >> 3];
      w = st[3][tid & 7];
    } else if (tid < 72) {      // db1[k]
      u = st[2][tid - 64];
    } else if (tid < 136) {      // dW2[o][k] = sum dy_o h_k
      u = st[0][(tid - 72) >> 3];
      w = st[1][(tid - 72) & 7];
    } else {      // db2[o]
      u = st[0][tid - 136];
    }
    float acc = 0.f;
    if (w)
      for (int i = 0; i < ST_THREADS; ++i) acc = fmaf(u[i], w[i], acc);
    else
      for (int i = 0; i < ST_THREADS; ++i) acc += u[i];
    part[(long)blockIdx.x * ST_TOK + tid] = acc;
  }
}

// The same two kernels for every other clip length 2 <= L <= ST_LMAX (args.seq_len up to 16, as the MFM teacher takes): L is a template
// argument, so the per-lane arrays a / h / g / dh [L] stay in registers; the form (one lane per (video, channel), both L x L weights and
// the biases in LDS) and the arithmetic (fmaf chains in index order, (acc + b2) + a) are those of the 8-frame kernels above, which
// L == 8 keeps.
template <int L>
struct TokWL {
  float w1[L][L], b1[L], w2[L][L], b2[L];
};
template <int L>
__device__ __forceinline__ void tok_load_l(TokWL<L>* s, const float* w1, const float* b1, const float* w2, const float* b2) {
  const int t = threadIdx.x;
  static_assert(L * L <= ST_THREADS, "one weight per lane");
  if (t < L * L) {
    (&s->w1[0][0])[t] = w1[t];
    (&s->w2[0][0])[t] = w2[t];
  }
  if (t < L) {
    s->b1[t] = b1[t];
    s->b2[t] = b2[t];
  }
  __syncthreads();
}

template <int L>
__global__ __launch_bounds__(ST_THREADS) void strm_tokmlp_fwd_l_k(const float* __restrict__ x, const float* __restrict__ pe,
                                                                   const float* __restrict__ mask, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                                   const float* __restrict__ b2, float* __restrict__ xp,
                                                                   float* __restrict__ y, unsigned char* __restrict__ hmask, long V, int D) {
  __shared__ TokWL<L> s;
  tok_load_l<L>(&s, w1, b1, w2, b2);
  const long t = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= V * D) return;
  const long v = t / D;
  const int d = (int)(t % D);
  float a[L], h[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const long at = (v * L + l) * D + d;
    float u = x[at] + pe[l * D + d];
    if (mask) u *= mask[at];
    a[l] = u;
    xp[at] = u;
  }
#pragma unroll
  for (int k = 0; k < L; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) acc = fmaf(s.w1[k][l], a[l], acc);
    h[k] = fmaxf(acc + s.b1[k], 0.f);
    if (hmask) hmask[(v * L + k) * D + d] = h[k] > 0.f;
  }
#pragma unroll
  for (int o = 0; o < L; ++o) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < L; ++k) acc = fmaf(s.w2[o][k], h[k], acc);
    y[(v * L + o) * D + d] = (acc + s.b2[o]) + a[o];
  }
}

// part[blockIdx.x][dW1 [L][L] | db1 [L] | dW2 [L][L] | db2 [L]]: 2 L^2 + 2 L outputs (544 at L = 16) over 256 lanes, so lane t reduces
// outputs t, t + 256, t + 512 one after the other, each over the 256 staged lanes in lane order.  The staging rows carry one pad float:
// lanes that reduce different rows at the same position then read different LDS banks (unpadded, every row starts on bank 0).
template <int L>
__global__ __launch_bounds__(ST_THREADS) void strm_tokmlp_bwd_l_k(const float* __restrict__ dy, const float* __restrict__ xp,
                                                                   const float* __restrict__ mask, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                                   float* __restrict__ dx, float* __restrict__ part, long V, int D) {
  constexpr int NT = 2 * L * L + 2 * L;
  __shared__ TokWL<L> s;
  __shared__ float st[4][L][ST_THREADS + 1];      // dy | h | masked dh | xp of every lane
  tok_load_l<L>(&s, w1, b1, w2, b1);
  const int tid = threadIdx.x;
  const long t = (long)blockIdx.x * ST_THREADS + tid;
  const bool live = t < V * D;
  const long v = live ? t / D : 0;
  const int d = live ? (int)(t % D) : 0;
  float a[L], h[L], g[L], dh[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const long at = (v * L + l) * D + d;
    a[l] = live ? xp[at] : 0.f;
    g[l] = live ? dy[at] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < L; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < L; ++l) acc = fmaf(s.w1[k][l], a[l], acc);
    h[k] = live ? fmaxf(acc + s.b1[k], 0.f) : 0.f;
  }
#pragma unroll
  for (int k = 0; k < L; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < L; ++o) acc = fmaf(s.w2[o][k], g[o], acc);
    dh[k] = h[k] > 0.f ? acc : 0.f;
  }
#pragma unroll
  for (int l = 0; l < L; ++l) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < L; ++k) acc = fmaf(s.w1[k][l], dh[k], acc);
    if (live) {
      const long at = (v * L + l) * D + d;
      float r = g[l] + acc;
      if (mask) r *= mask[at];
      dx[at] = r;
    }
    st[0][l][tid] = g[l];
    st[1][l][tid] = h[l];
    st[2][l][tid] = dh[l];
    st[3][l][tid] = a[l];
  }
  __syncthreads();
  for (int o = tid; o < NT; o += ST_THREADS) {
    const float *u, *w = nullptr;
    if (o < L * L) {      // dW1[k][l] = sum dh_k xp_l
      u = st[2][o / L];
      w = st[3][o % L];
    } else if (o < L * L + L) {      // db1[k]
      u = st[2][o - L * L];
    } else if (o < 2 * L * L + L) {      // dW2[o][k] = sum dy_o h_k
      u = st[0][(o - L * L - L) / L];
      w = st[1][(o - L * L - L) % L];
    } else {      // db2[o]
      u = st[0][o - 2 * L * L - L];
    }
    float acc = 0.f;
    if (w)
      for (int i = 0; i < ST_THREADS; ++i) acc = fmaf(u[i], w[i], acc);
    else
      for (int i = 0; i < ST_THREADS; ++i) acc += u[i];
    part[(long)blockIdx.x * NT + o] = acc;
  }
}

#define ST_L_CASE(N, ...)    \
  case N: {                  \
    constexpr int Lc = N;    \
    __VA_ARGS__;             \
  } break;
// every clip length but 8 (which has its own kernels): Lc is the compile-time length inside the statement
#define ST_DISPATCH_L(LV, ...)                                                                                                        \
  switch (LV) {                                                                                                                       \
    ST_L_CASE(2, __VA_ARGS__) ST_L_CASE(3, __VA_ARGS__) ST_L_CASE(4, __VA_ARGS__) ST_L_CASE(5, __VA_ARGS__) ST_L_CASE(6, __VA_ARGS__)  \
    ST_L_CASE(7, __VA_ARGS__) ST_L_CASE(9, __VA_ARGS__) ST_L_CASE(10, __VA_ARGS__) ST_L_CASE(11, __VA_ARGS__)                          \
    ST_L_CASE(12, __VA_ARGS__) ST_L_CASE(13, __VA_ARGS__) ST_L_CASE(14, __VA_ARGS__) ST_L_CASE(15, __VA_ARGS__)                        \
    ST_L_CASE(16, __VA_ARGS__)                                                                                                        \
    default: break;                                                                                                                   \
  }

extern "C" long lmkd_strm_tokmlp_parts(long V, int D) { return V > 0 && D > 0 ? (V * D + ST_THREADS - 1) / ST_THREADS : 0; }

extern "C" int lmkd_strm_tokmlp_fwd(const float* x, const float* pe, const float* mask, const float* w1, const float* b1, const float* w2,
                                    const float* b2, float* xp, float* y, unsigned char* hmask, int V, int L, int D, void* stream) {
  LMKD_REQUIRE(x && pe && w1 && b1 && w2 && b2 && xp && y && V > 0 && D > 0, "lmkd_strm_tokmlp_fwd: bad arguments");
  LMKD_REQUIRE(L >= 2 && L <= ST_LMAX, "lmkd_strm_tokmlp_fwd: the token MLP takes 2 <= L <= %d frames per video, got %d", ST_LMAX, L);
  const dim3 grid(st_grid((long)V * D));
  if (L == ST_L) {
    hipLaunchKernelGGL(strm_tokmlp_fwd_k, grid, dim3(ST_THREADS), 0, (hipStream_t)stream, x, pe, mask, w1, b1, w2, b2, xp, y, hmask, (long)V, D);
  } else {
    ST_DISPATCH_L(L, hipLaunchKernelGGL((strm_tokmlp_fwd_l_k<Lc>), grid, dim3(ST_THREADS), 0, (hipStream_t)stream, x, pe, mask, w1, b1, w2, b2,
                                         xp, y, hmask, (long)V, D));
  }
  LMKD_CHECK_LAUNCH("strm_tokmlp_fwd_k");
  return LMKD_OK;
}

/* dparams [2 L^2 + 2 L] = dW1 | db1 | dW2 | db2; part: lmkd_strm_tokmlp_parts(V, D) rows of 2 L^2 + 2 L floats */
extern "C" int lmkd_strm_tokmlp_bwd(const float* dy, const float* xp, const float* mask, const float* w1, const float* b1, const float* w2,
                                    float* dx, float* part, float* dparams, int V, int L, int D, void* stream) {
  LMKD_REQUIRE(dy && xp && w1 && b1 && w2 && dx && part && dparams && V > 0 && D > 0, "lmkd_strm_tokmlp_bwd: bad arguments");
  LMKD_REQUIRE(L >= 2 && L <= ST_LMAX, "lmkd_strm_tokmlp_bwd: the token MLP takes 2 <= L <= %d frames per video, got %d", ST_LMAX, L);
  const int nb = st_grid((long)V * D), nt = 2 * L * L + 2 * L;
  if (L == ST_L) {
    hipLaunchKernelGGL(strm_tokmlp_bwd_k, dim3(nb), dim3(ST_THREADS), 0, (hipStream_t)stream, dy, xp, mask, w1, b1, w2, dx, part, (long)V, D);
  } else {
    ST_DISPATCH_L(L, hipLaunchKernelGGL((strm_tokmlp_bwd_l_k<Lc>), dim3(nb), dim3(ST_THREADS), 0, (hipStream_t)stream, dy, xp, mask, w1, b1, w2,
                                         dx, part, (long)V, D));
  }
  LMKD_CHECK_LAUNCH("strm_tokmlp_bwd_k");
  hipLaunchKernelGGL(strm_reduce_rows_k, dim3(nt), dim3(ST_THREADS), 0, (hipStream_t)stream, part, dparams, nb, nt);
  LMKD_CHECK_LAUNCH("strm_reduce_rows_k");
  return LMKD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// patch-distance head (DistanceLoss).  P [NV * L][2 Hd] = per-frame projections (first-frame half | second-frame half of clsW)
// ------------------------------------------------------------------------------------------------------------------------------------
// pair index of frames i < j in itertools.combinations order
__device__ __forceinline__ int pair_at(int i, int j, int L) { return i * L - (i * (i + 1)) / 2 + (j - i - 1); }

// E[v, t(i,j), :] = relu(P_a[v, i] + P_b[v, j] + b)
__global__ void strm_pair_embed_k(const float* __restrict__ P, const float* __restrict__ b, float* __restrict__ E, long NV, int L, int Hd) {
  const int H4 = Hd >> 2, T = L * (L - 1) / 2;
  const long t = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= NV * T * H4) return;
  const int k = (int)(t % H4) * 4;
  int p = (int)((t / H4) % T);
  const long v = t / ((long)H4 * T);
  int i = 0;
  while (p >= L - 1 - i) {
    p -= L - 1 - i;
    ++i;
  }
  const int j = i + 1 + p;
  const float4 a = sld4(P + (v * L + i) * 2 * Hd + k), c = sld4(P + (v * L + j) * 2 * Hd + Hd + k), e = sld4(b + k);
  sst4(E + t * 4, make_float4(fmaxf((a.x + c.x) + e.x, 0.f), fmaxf((a.y + c.y) + e.y, 0.f), fmaxf((a.z + c.z) + e.z, 0.f),
                              fmaxf((a.w + c.w) + e.w, 0.f)));
}

// One wave per (ST_QR query pair rows, class): the query rows stay in registers (lane l holds columns 4 l + 256 m), every pair row of the
// class's support videos is read once, squared differences are summed per lane and across the wave by an xor butterfly (all lanes end with
// the same sum), the first smallest wins.  order[c * shot + m] = support video of member m of class c (labels ascending, videos ascending).
__global__ __launch_bounds__(64) void strm_mindist_k(const float* __restrict__ E, const int* __restrict__ order, float* __restrict__ dist,
                                                      int* __restrict__ idx, int Ns, int Nq, int way, int shot, int T) {
  const int lane = threadIdx.x, c = blockIdx.y;
  const int R = Nq * T, r0 = blockIdx.x * ST_QR;
  float4 q[ST_QR][4];
#pragma unroll
  for (int r = 0; r < ST_QR; ++r) {
    const int row = min(r0 + r, R - 1);
    const float* e = E + ((long)Ns * T + row) * ST_HD + lane * 4;
#pragma unroll
    for (int m = 0; m < 4; ++m) q[r][m] = sld4(e + m * 256);
  }
  float best[ST_QR];
  int bi[ST_QR];
#pragma unroll
  for (int r = 0; r < ST_QR; ++r) {
    best[r] = INFINITY;
    bi[r] = 0;
  }
  for (int mem = 0; mem < shot; ++mem) {
    const int sv = order[c * shot + mem];
    for (int t = 0; t < T; ++t) {
      const float* e = E + ((long)sv * T + t) * ST_HD + lane * 4;
      float4 s[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) s[m] = sld4(e + m * 256);
#pragma unroll
      for (int r = 0; r < ST_QR; ++r) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float dx = q[r][m].x - s[m].x, dy = q[r][m].y - s[m].y, dz = q[r][m].z - s[m].z, dw = q[r][m].w - s[m].w;
          a.x = fmaf(dx, dx, a.x);
          a.y = fmaf(dy, dy, a.y);
          a.z = fmaf(dz, dz, a.z);
          a.w = fmaf(dw, dw, a.w);
        }
        float d2 = (a.x + a.y) + (a.z + a.w);
        for (int o = 32; o > 0; o >>= 1) d2 += __shfl_xor(d2, o, 64);
        if (d2 < best[r]) {
          best[r] = d2;
          bi[r] = mem * T + t;
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < ST_QR; ++r)
      if (r0 + r < R) {
        dist[(long)(r0 + r) * way + c] = sqrtf(best[r]);
        idx[(long)(r0 + r) * way + c] = bi[r];
      }
  }
}

// The same minimum for long clips (the work grows with T^2): one workgroup of four waves per (4 ST_QR = 16 query pair rows, class).  Wave w
// keeps query rows 4 w .. 4 w + 3 in registers as above; the class's support pair rows pass through LDS in blocks of ST_SB rows, so a row
// is fetched from global memory once per workgroup and read from LDS once per wave.  The distance of one (query row, support row) is the
// arithmetic of strm_mindist_k: direct differences, lane l on columns 4 l + 256 m, one fmaf chain over m per component,
// (x + y) + (z + w), and the xor butterfly 32, 16, .. 1.  The butterfly runs transposed over the 8 sums of (4 query rows, 2 support rows):
// at offsets 32, 16 and 8 a lane keeps half of its sums and hands the other half to its partner, which adds the same two operands the
// plain butterfly adds (own + partner's, in either order), so after three steps lanes 8 j .. 8 j + 7 hold sum j = 2 r + s reduced over
// offsets 32, 16, 8 and three ordinary steps finish it: 10 exchanges for 8 sums instead of 48, the same tree, the same bits.  Candidates
// are then visited in (member, t) order with strict <, every lane of query row r's 16 lanes alike.
__global__ __launch_bounds__(ST_THREADS) void strm_mindist_tile_k(const float* __restrict__ E, const int* __restrict__ order,
                                                                   float* __restrict__ dist, int* __restrict__ idx, int Ns, int Nq, int way,
                                                                   int shot, int T) {
  __shared__ __attribute__((aligned(16))) float S[ST_SB][ST_HD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.y;
  const int R = Nq * T, r0 = blockIdx.x * (4 * ST_QR) + wave * ST_QR, NS = shot * T;
  float4 q[ST_QR][4];
#pragma unroll
  for (int r = 0; r < ST_QR; ++r) {
    const int row = min(r0 + r, R - 1);
    const float* e = E + ((long)Ns * T + row) * ST_HD + lane * 4;
#pragma unroll
    for (int m = 0; m < 4; ++m) q[r][m] = sld4(e + m * 256);
  }
  float best = INFINITY;      // of query row r0 + (lane >> 4)
  int bi = 0;
  const bool up32 = lane & 32, up16 = lane & 16, up8 = lane & 8;
  for (int g0 = 0; g0 < NS; g0 += ST_SB) {
    const int nb = min(ST_SB, NS - g0);
    __syncthreads();      // the previous block has been read by every wave
    for (int b = 0; b < nb; ++b) {
      const int g = g0 + b, sv = order[c * shot + g / T];
      sst4(&S[b][tid * 4], sld4(E + ((long)sv * T + g % T) * ST_HD + tid * 4));
    }
    __syncthreads();
    for (int b = 0; b < nb; b += 2) {
      const bool two = b + 1 < nb;
      const float* s0 = &S[b][lane * 4];
      const float* s1 = &S[two ? b + 1 : b][lane * 4];
      float4 a[ST_QR][2];
#pragma unroll
      for (int r = 0; r < ST_QR; ++r) a[r][0] = a[r][1] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float4 u0 = sld4(s0 + m * 256), u1 = sld4(s1 + m * 256);
#pragma unroll
        for (int r = 0; r < ST_QR; ++r) {
          {
            const float dx = q[r][m].x - u0.x, dy = q[r][m].y - u0.y, dz = q[r][m].z - u0.z, dw = q[r][m].w - u0.w;
            a[r][0].x = fmaf(dx, dx, a[r][0].x);
            a[r][0].y = fmaf(dy, dy, a[r][0].y);
            a[r][0].z = fmaf(dz, dz, a[r][0].z);
            a[r][0].w = fmaf(dw, dw, a[r][0].w);
          }
          {
            const float dx = q[r][m].x - u1.x, dy = q[r][m].y - u1.y, dz = q[r][m].z - u1.z, dw = q[r][m].w - u1.w;
            a[r][1].x = fmaf(dx, dx, a[r][1].x);
            a[r][1].y = fmaf(dy, dy, a[r][1].y);
            a[r][1].z = fmaf(dz, dz, a[r][1].z);
            a[r][1].w = fmaf(dw, dw, a[r][1].w);
          }
        }
      }
      float v8[8];      // sum j = 2 r + s
#pragma unroll
      for (int r = 0; r < ST_QR; ++r)
#pragma unroll
        for (int s = 0; s < 2; ++s) v8[2 * r + s] = (a[r][s].x + a[r][s].y) + (a[r][s].z + a[r][s].w);
      float v4[4], v2[2];
#pragma unroll
      for (int k = 0; k < 4; ++k) {      // lanes 32.. keep sums 4..7
        const float keep = up32 ? v8[k + 4] : v8[k], give = up32 ? v8[k] : v8[k + 4];
        v4[k] = keep + __shfl_xor(give, 32, 64);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float keep = up16 ? v4[k + 2] : v4[k], give = up16 ? v4[k] : v4[k + 2];
        v2[k] = keep + __shfl_xor(give, 16, 64);
      }
      const float keep = up8 ? v2[1] : v2[0], give = up8 ? v2[0] : v2[1];
      float d2 = keep + __shfl_xor(give, 8, 64);
      for (int o = 4; o > 0; o >>= 1) d2 += __shfl_xor(d2, o, 64);
      // this lane: query row lane >> 4, support row b + ((lane >> 3) & 1); the other support row's sum sits 8 lanes away
      const float other = __shfl_xor(d2, 8, 64);
      const float d0 = up8 ? other : d2, d1 = up8 ? d2 : other;
      if (d0 < best) {
        best = d0;
        bi = g0 + b;
      }
      if (two && d1 < best) {
        best = d1;
        bi = g0 + b + 1;
      }
    }
  }
  const int row = r0 + (lane >> 4);
  if ((lane & 15) == 0 && row < R) {
    dist[(long)row * way + c] = sqrtf(best);
    idx[(long)row * way + c] = bi;
  }
}

// logits[q, c] = - mean over the T pair rows of the minimum distance
__global__ void strm_dist_logits_k(const float* __restrict__ dist, float* __restrict__ out, int Nq, int way, int T) {
  const int t = blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= Nq * way) return;
  const int q = t / way, c = t % way;
  float s = 0.f;
  for (int p = 0; p < T; ++p) s += dist[((long)q * T + p) * way + c];
  out[t] = -(s / (float)T);
}

// d loss / d (pre-ReLU pair embedding), one workgroup per pair row of E.  A query row owns its `way` terms; a support row scans the query
// rows' selections of its own class in row order.  d |q - s| / dq = (q - s) / |q - s|, 0 at distance 0 (as cdist's backward).
// pos[v] = class-sorted position of support video v ( = class * shot + member).
__global__ __launch_bounds__(ST_THREADS) void strm_mindist_bwd_k(const float* __restrict__ E, const int* __restrict__ order,
                                                                  const int* __restrict__ pos, const float* __restrict__ dist,
                                                                  const int* __restrict__ idx, const float* __restrict__ g,
                                                                  float* __restrict__ dpre, int Ns, int Nq, int way, int shot, int T) {
  const long row = blockIdx.x;
  const int k = threadIdx.x * 4;
  const float4 me = sld4(E + row * ST_HD + k);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const float invT = 1.f / (float)T;
  if (row >= (long)Ns * T) {
    const int r = (int)(row - (long)Ns * T), qv = r / T;
    for (int c = 0; c < way; ++c) {
      const float d = dist[(long)r * way + c];
      if (!(d > 0.f)) continue;
      const int sel = idx[(long)r * way + c];
      if (sel < 0 || sel >= shot * T) continue;      // selections are an input of the backward: never index outside the class
      const int sv = order[c * shot + sel / T];
      const float4 o = sld4(E + ((long)sv * T + sel % T) * ST_HD + k);
      const float coef = -(g[qv * way + c] * invT) / d;
      acc.x = fmaf(coef, me.x - o.x, acc.x);
      acc.y = fmaf(coef, me.y - o.y, acc.y);
      acc.z = fmaf(coef, me.z - o.z, acc.z);
      acc.w = fmaf(coef, me.w - o.w, acc.w);
    }
  } else {
    const int v = (int)(row / T), p = pos[v], c = p / shot, mine = (p % shot) * T + (int)(row % T);
    for (int r = 0; r < Nq * T; ++r) {
      if (idx[(long)r * way + c] != mine) continue;
      const float d = dist[(long)r * way + c];
      if (!(d > 0.f)) continue;
      const float4 o = sld4(E + ((long)Ns * T + r) * ST_HD + k);
      const float coef = -(g[(r / T) * way + c] * invT) / d;
      acc.x = fmaf(coef, me.x - o.x, acc.x);      // -coef (q - s) = coef (s - q)
      acc.y = fmaf(coef, me.y - o.y, acc.y);
      acc.z = fmaf(coef, me.z - o.z, acc.z);
      acc.w = fmaf(coef, me.w - o.w, acc.w);
    }
  }
  sst4(dpre + row * ST_HD + k, make_float4(me.x > 0.f ? acc.x : 0.f, me.y > 0.f ? acc.y : 0.f, me.z > 0.f ? acc.z : 0.f, me.w > 0.f ? acc.w : 0.f));
}

// dP[v, f, :Hd] = sum over pairs (f, j > f) of dpre, dP[v, f, Hd:] = sum over pairs (i < f, f): a gather in pair order
__global__ void strm_pair_gather_k(const float* __restrict__ dpre, float* __restrict__ dP, long NV, int L, int Hd) {
  const int H4 = Hd >> 2, T = L * (L - 1) / 2;
  const long t = (long)blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= NV * L * H4) return;
  const int k = (int)(t % H4) * 4, f = (int)((t / H4) % L);
  const long v = t / ((long)H4 * L);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  for (int j = f + 1; j < L; ++j) {
    const float4 u = sld4(dpre + (v * T + pair_at(f, j, L)) * Hd + k);
    a = make_float4(a.x + u.x, a.y + u.y, a.z + u.z, a.w + u.w);
  }
  for (int i = 0; i < f; ++i) {
    const float4 u = sld4(dpre + (v * T + pair_at(i, f, L)) * Hd + k);
    b = make_float4(b.x + u.x, b.y + u.y, b.z + u.z, b.w + u.w);
  }
  sst4(dP + (v * L + f) * 2 * Hd + k, a);
  sst4(dP + (v * L + f) * 2 * Hd + Hd + k, b);
}

static int dist_check(const char* who, int Ns, int Nq, int way, int shot, int L, int Hd) {
  LMKD_REQUIRE(Ns > 0 && Nq > 0 && way > 0 && shot > 0 && Ns == way * shot && L >= 2 && L <= 16,
               "%s: needs Ns == way * shot (every class with `shot` support videos) and 2 <= L <= 16, got Ns %d way %d shot %d L %d", who, Ns,
               way, shot, L);
  LMKD_REQUIRE(Hd == ST_HD, "%s: built for %d-wide pair embeddings, got %d", who, ST_HD, Hd);
  return LMKD_OK;
}

extern "C" int lmkd_strm_pair_embed(const float* P, const float* bias, float* E, int NV, int L, int Hd, void* stream) {
  LMKD_REQUIRE(P && bias && E && NV > 0 && L >= 2 && L <= 16 && Hd > 0 && Hd % 4 == 0 && aligned16(P) && aligned16(bias) && aligned16(E),
               "lmkd_strm_pair_embed: bad arguments");
  const int T = L * (L - 1) / 2;
  hipLaunchKernelGGL(strm_pair_embed_k, dim3(st_grid((long)NV * T * (Hd / 4))), dim3(ST_THREADS), 0, (hipStream_t)stream, P, bias, E, (long)NV, L,
                     Hd);
  LMKD_CHECK_LAUNCH("strm_pair_embed_k");
  return LMKD_OK;
}

// which minimum-distance kernel lmkd_strm_patchdist_fwd launches: -1 = the measured dispatch, 0 = never the tiled one, 1 = always (A/B runs
// and tests; both give the same bits)
static int g_pd_tiled = -1;
extern "C" int lmkd_patchdist_set_tiled(int mode) {
  LMKD_REQUIRE(mode >= -1 && mode <= 1, "lmkd_patchdist_set_tiled: mode must be -1 (measured dispatch), 0 (never) or 1 (always), got %d", mode);
  g_pd_tiled = mode;
  return LMKD_OK;
}

extern "C" int lmkd_strm_patchdist_fwd(const float* E, const int* order, float* dist, int* idx, float* logits, int Ns, int Nq, int way, int shot,
                                       int L, int Hd, void* stream) {
  if (int rc = dist_check("lmkd_strm_patchdist_fwd", Ns, Nq, way, shot, L, Hd)) return rc;
  LMKD_REQUIRE(E && order && dist && idx && logits && aligned16(E), "lmkd_strm_patchdist_fwd: null or unaligned tensor");
  const int T = L * (L - 1) / 2;
  // measured dispatch (profiles/strm_long_bench.json): clips of up to 8 frames keep the one-wave kernel
  if (g_pd_tiled == 1 || (g_pd_tiled < 0 && L > ST_L)) {
    hipLaunchKernelGGL(strm_mindist_tile_k, dim3((Nq * T + 4 * ST_QR - 1) / (4 * ST_QR), way), dim3(ST_THREADS), 0, (hipStream_t)stream, E, order,
                       dist, idx, Ns, Nq, way, shot, T);
    LMKD_CHECK_LAUNCH("strm_mindist_tile_k");
  } else {
    hipLaunchKernelGGL(strm_mindist_k, dim3((Nq * T + ST_QR - 1) / ST_QR, way), dim3(64), 0, (hipStream_t)stream, E, order, dist, idx, Ns, Nq,
                       way, shot, T);
    LMKD_CHECK_LAUNCH("strm_mindist_k");
  }
  hipLaunchKernelGGL(strm_dist_logits_k, dim3(st_grid((long)Nq * way)), dim3(ST_THREADS), 0, (hipStream_t)stream, dist, logits, Nq, way, T);
  LMKD_CHECK_LAUNCH("strm_dist_logits_k");
  return LMKD_OK;
}

/* g [Nq, way] -> dP [NV * L][2 Hd] (gradient of the per-frame projections) and dpre [NV * T][Hd] (gradient before the ReLU; its column
   sum is the bias gradient) */
extern "C" int lmkd_strm_patchdist_bwd(const float* E, const int* order, const int* pos, const float* dist, const int* idx, const float* g,
                                       float* dpre, float* dP, int Ns, int Nq, int way, int shot, int L, int Hd, void* stream) {
  if (int rc = dist_check("lmkd_strm_patchdist_bwd", Ns, Nq, way, shot, L, Hd)) return rc;
  LMKD_REQUIRE(E && order && pos && dist && idx && g && dpre && dP && aligned16(E) && aligned16(dpre) && aligned16(dP),
               "lmkd_strm_patchdist_bwd: null or unaligned tensor");
  const int T = L * (L - 1) / 2, NV = Ns + Nq;
  hipLaunchKernelGGL(strm_mindist_bwd_k, dim3(NV * T), dim3(ST_THREADS), 0, (hipStream_t)stream, E, order, pos, dist, idx, g, dpre, Ns, Nq, way,
                     shot, T);
  LMKD_CHECK_LAUNCH("strm_mindist_bwd_k");
  hipLaunchKernelGGL(strm_pair_gather_k, dim3(st_grid((long)NV * L * (Hd / 4))), dim3(ST_THREADS), 0, (hipStream_t)stream, dpre, dP, (long)NV, L, Hd);
  LMKD_CHECK_LAUNCH("strm_pair_gather_k");
  return LMKD_OK;
}
