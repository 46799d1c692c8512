// MobileNetV3-Large student trunk (torchvision mobilenet_v3_large().features, the `mobile` module of
// model/backbone/moblienetv3.py:26-31): depthwise k x k convolutions, the 3 x 3 / stride-2 stem on the NHWC4 input, BatchNorm +
// {none, ReLU, Hardswish} (+ residual) with its train-mode backward, and the squeeze-excitation pieces.  The 1 x 1 convolutions are
// GEMMs on lmkd_gemm_f32; their BatchNorm statistics come from lmkd_col_stats.
//
// All tensors NHWC fp32 with C % 8 == 0 (the network's widths are multiples of 8, not of 32: 16, 24, 40, 72, 120, 184, 200, ...).
// Plain fp32 FMA-free arithmetic (-ffp-contract=off, like the rest of the library) with fp32 accumulation (the BatchNorm backward's tile
// sums in double); every reduction is a fixed-order
// two-level one - per-workgroup partials into a [T][...] buffer, then col_reduce_kernel (or lmkd_bn_finalize) over T in double in a
// fixed order - so every result is run-to-run bit-identical.  No float atomics.
//
// Thread layout of the per-pixel kernels: a 256-lane workgroup is CL channel lanes (4 channels each, one 16-byte access) x PL = 256 / CL
// pixel lanes, CL = 8 when C % 32 == 0, 4 when C % 16 == 0, else 2, so no lane idles at any width; grid.y walks channel groups of 4 CL.
#include "common.h"
#include <algorithm>

#define MN_THREADS 256
#define MN_TILE_STAT 1024      // output pixels per workgroup of the statistics-producing kernels: rows of the [T][C][2] partial buffer
#define MN_TILE_RED 4096       // pixels per workgroup of the weight-gradient / BatchNorm-backward reductions

static inline int mn_cl(int C) { return C % 32 == 0 ? 8 : (C % 16 == 0 ? 4 : 2); }

extern "C" long lmkd_mnv3_stat_tiles(long pixels) { return pixels > 0 ? (pixels + MN_TILE_STAT - 1) / MN_TILE_STAT : 0; }

static inline long red_tiles(long pixels) { return (pixels + MN_TILE_RED - 1) / MN_TILE_RED; }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float f4get(const float4& v, int q) { return q == 0 ? v.x : (q == 1 ? v.y : (q == 2 ? v.z : v.w)); }

// aten's CPU kernels (BinaryOpsKernel / Activation.cpp): hardswish(x) = x min(max(x + 3, 0), 6) / 6, derivative 0 for x <= -3,
// x / 3 + 1/2 on (-3, 3), 1 for x >= 3; hardsigmoid(x) = min(max(x + 3, 0), 6) / 6, derivative 1/6 on (-3, 3), else 0
__device__ __forceinline__ float act_fwd(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f;
  return v;
}
__device__ __forceinline__ float act_bwd(float v, float g, int act) {
  if (act == 1) return v > 0.f ? g : 0.f;
  if (act == 2) return v <= -3.f ? 0.f : (v < 3.f ? g * (v / 3.f + 0.5f) : g);
  return g;
}

// Sums of the PL pixel lanes of a workgroup for NV values per channel lane (4 channels each), in LDS, fixed order.
// vals[k][q]: value k of channel q of this lane.  Result for (k, channel cc of the group) returned through `out(k, cc, sum)` by lanes
// tid < NV * 4 CL.
template <int CL, int NV, typename V, typename Out>
__device__ __forceinline__ void lane_reduce(V (*vals)[4], V* red, Out out) {
  constexpr int PL = MN_THREADS / CL;
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
#pragma unroll
  for (int k = 0; k < NV; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) red[(k * PL + pl) * (4 * CL) + cl * 4 + q] = vals[k][q];
  __syncthreads();
  for (int col = tid; col < NV * 4 * CL; col += MN_THREADS) {
    const int k = col / (4 * CL), cc = col % (4 * CL);
    V s = 0;
    for (int p = 0; p < PL; ++p) s += red[(k * PL + p) * (4 * CL) + cc];
    out(k, cc, s);
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------
// fixed-order column reduction of a [T][NC] partial buffer: out[c] = (accumulate ? out[c] : 0) + sum_t part[t][c], double accumulation.
// 32 columns x 8 row lanes per workgroup; row lane r sums rows r, r + 8, ... (four interleaved accumulators), then lane 0 adds the eight.
// ---------------------------------------------------------------------------------
template <typename V>
__global__ void __launch_bounds__(256) col_reduce_kernel(const V* __restrict__ part, long T, long NC, float* __restrict__ out, int accumulate) {
  __shared__ double sm[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long c = (long)blockIdx.x * 32 + tx;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < NC) {
    long t = ty;
    for (; t + 24 < T; t += 32) {
      a0 += (double)part[t * NC + c];
      a1 += (double)part[(t + 8) * NC + c];
      a2 += (double)part[(t + 16) * NC + c];
      a3 += (double)part[(t + 24) * NC + c];
    }
    for (; t < T; t += 8) a0 += (double)part[t * NC + c];
  }
  sm[ty][tx] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (ty == 0 && c < NC) {
    double s = 0.0;
    for (int r = 0; r < 8; ++r) s += sm[r][tx];
    out[c] = (accumulate ? out[c] : 0.f) + (float)s;
  }
}
template <typename V>
static int col_reduce(const V* part, long T, long NC, float* out, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(col_reduce_kernel<V>, dim3(cdiv(NC, 32)), dim3(256), 0, st, part, T, NC, out, accumulate);
  LMKD_CHECK_LAUNCH("col_reduce_kernel");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// depthwise K x K convolution, stride S, pad (K - 1) / 2 (torchvision InvertedResidual's groups = C ConvBNActivation).
// w: [C][K][K] (OIHW of the [C, 1, K, K] parameter).  Forward: one output pixel x 4 channels per lane per step, the lane's K K x 4 weights
// in registers for the whole tile, the k x k input reads of neighbouring output pixels shared through L1 / L2; the epilogue leaves the
// BatchNorm partial sums (sum, sum of squares) of the tile in part[tile][C][2] (lmkd_bn_finalize reads it).
// ---------------------------------------------------------------------------------
template <int CL, int K>
__global__ void __launch_bounds__(MN_THREADS) dw_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                            float* __restrict__ part, int N, int H, int W, int C, int S, int Ho, int Wo) {
  constexpr int PL = MN_THREADS / CL, KK = K * K, P = (K - 1) / 2;
  __shared__ float red[2 * MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  float wr[KK][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < KK; ++t) wr[t][q] = w[(long)(c0 + q) * KK + t];
  const long npix = (long)N * Ho * Wo;
  const long p0 = (long)blockIdx.x * MN_TILE_STAT;
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i = pl; i < MN_TILE_STAT; i += PL) {
    const long p = p0 + i;
    if (p >= npix) break;
    const int ow = (int)(p % Wo);
    const long r = p / Wo;
    const int oh = (int)(r % Ho);
    const long n = r / Ho;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int ih = oh * S - P + kh;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const int iw = ow * S - P + kw;
        if (iw < 0 || iw >= W) continue;
        const float4 v = ld4(x + ((n * H + ih) * W + iw) * C + c0);
        o[0] += v.x * wr[kh * K + kw][0];
        o[1] += v.y * wr[kh * K + kw][1];
        o[2] += v.z * wr[kh * K + kw][2];
        o[3] += v.w * wr[kh * K + kw][3];
      }
    }
    st4(y + p * C + c0, make_float4(o[0], o[1], o[2], o[3]));
#pragma unroll
    for (int q = 0; q < 4; ++q) { acc[0][q] += o[q]; acc[1][q] += o[q] * o[q]; }
  }
  if (!part) return;      // uniform over the workgroup
  float* pt = part + (long)blockIdx.x * C * 2 + (long)blockIdx.y * 4 * CL * 2;
  lane_reduce<CL, 2>(acc, red, [&](int k, int cc, float s) { pt[cc * 2 + k] = s; });
}

// data gradient, gather form: one input pixel x 4 channels per lane, dx = sum over the taps that reach it of dy * w
template <int CL, int K>
__global__ void __launch_bounds__(MN_THREADS) dw_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                              long npix, int H, int W, int C, int S, int Ho, int Wo) {
  constexpr int PL = MN_THREADS / CL, KK = K * K, P = (K - 1) / 2;
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  float wr[KK][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < KK; ++t) wr[t][q] = w[(long)(c0 + q) * KK + t];
  for (long p = (long)blockIdx.x * PL + pl; p < npix; p += (long)gridDim.x * PL) {
    const int iw = (int)(p % W);
    const long r = p / W;
    const int ih = (int)(r % H);
    const long n = r / H;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int th = ih + P - kh;      // = oh * S
      if (th < 0 || th % S) continue;
      const int oh = th / S;
      if (oh >= Ho) continue;
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const int tw = iw + P - kw;
        if (tw < 0 || tw % S) continue;
        const int ow = tw / S;
        if (ow >= Wo) continue;
        const float4 g = ld4(dy + ((n * Ho + oh) * Wo + ow) * C + c0);
        o[0] += g.x * wr[kh * K + kw][0];
        o[1] += g.y * wr[kh * K + kw][1];
        o[2] += g.z * wr[kh * K + kw][2];
        o[3] += g.w * wr[kh * K + kw][3];
      }
    }
    st4(dx + p * C + c0, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// weight gradient: each lane keeps the K K x 4 products of its output pixels; the workgroup's sums over its MN_TILE_RED pixels go to
// part[tile][C][KK] (taps in groups of 8 through LDS), col_reduce_kernel adds the tiles: dw[c][t] (+)= sum over tiles
template <int CL, int K>
__global__ void __launch_bounds__(MN_THREADS) dw_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
                                                              int N, int H, int W, int C, int S, int Ho, int Wo) {
  constexpr int PL = MN_THREADS / CL, KK = K * K, P = (K - 1) / 2;
  __shared__ float red[8 * MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  const long npix = (long)N * Ho * Wo;
  const long p0 = (long)blockIdx.x * MN_TILE_RED;
  float acc[KK][4];
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[t][q] = 0.f;
  for (int i = pl; i < MN_TILE_RED; i += PL) {
    const long p = p0 + i;
    if (p >= npix) break;
    const int ow = (int)(p % Wo);
    const long r = p / Wo;
    const int oh = (int)(r % Ho);
    const long n = r / Ho;
    const float4 g = ld4(dy + p * C + c0);
#pragma unroll
    for (int kh = 0; kh < K; ++kh) {
      const int ih = oh * S - P + kh;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const int iw = ow * S - P + kw;
        if (iw < 0 || iw >= W) continue;
        const float4 v = ld4(x + ((n * H + ih) * W + iw) * C + c0);
        acc[kh * K + kw][0] += g.x * v.x;
        acc[kh * K + kw][1] += g.y * v.y;
        acc[kh * K + kw][2] += g.z * v.z;
        acc[kh * K + kw][3] += g.w * v.w;
      }
    }
  }
  float* pt = part + (long)blockIdx.x * C * KK + (long)blockIdx.y * 4 * CL * KK;
#pragma unroll
  for (int t0 = 0; t0 < KK; t0 += 8) {
    const int nt = KK - t0 < 8 ? KK - t0 : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(j * PL + pl) * (4 * CL) + cl * 4 + q] = acc[t0 + j < KK ? t0 + j : 0][q];
    __syncthreads();
    for (int col = tid; col < nt * 4 * CL; col += MN_THREADS) {
      const int j = col / (4 * CL), cc = col % (4 * CL);
      float s = 0.f;
      for (int pp = 0; pp < PL; ++pp) s += red[(j * PL + pp) * (4 * CL) + cc];
      pt[cc * KK + t0 + j] = s;
    }
    __syncthreads();
  }
}

#define MN_DISPATCH_CL(CLV, ...)                         \
  do {                                                   \
    if ((CLV) == 8) { constexpr int CLc = 8; __VA_ARGS__; } \
    else if ((CLV) == 4) { constexpr int CLc = 4; __VA_ARGS__; } \
    else { constexpr int CLc = 2; __VA_ARGS__; }          \
  } while (0)

static inline int dw_out(int H, int K, int S) { return (H + 2 * ((K - 1) / 2) - K) / S + 1; }

static const char* dw_check(int N, int H, int W, int C, int K, int S) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return "empty tensor";
  if (C % 8) return "C % 8 != 0";
  if (K != 3 && K != 5) return "kernel size must be 3 or 5";
  if (S != 1 && S != 2) return "stride must be 1 or 2";
  if ((long)N * H * W * C >= (1L << 31) * 4L) return "tensor too large";
  return nullptr;
}

extern "C" int lmkd_dw_conv_fwd(const float* x, const float* w, float* y, float* stat_partial, int N, int H, int W, int C, int K, int stride,
                                void* stream) {
  const char* e = dw_check(N, H, W, C, K, stride);
  LMKD_REQUIRE(!e, "lmkd_dw_conv_fwd: %s (N=%d H=%d W=%d C=%d K=%d stride=%d)", e ? e : "", N, H, W, C, K, stride);
  LMKD_REQUIRE(x && w && y && aligned16(x) && aligned16(y), "lmkd_dw_conv_fwd: null or unaligned pointer");
  const int Ho = dw_out(H, K, stride), Wo = dw_out(W, K, stride), CL = mn_cl(C);
  const dim3 grid((unsigned)lmkd_mnv3_stat_tiles((long)N * Ho * Wo), C / (4 * CL));
  MN_DISPATCH_CL(CL, {
    if (K == 3) hipLaunchKernelGGL((dw_fwd_kernel<CLc, 3>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, x, w, y, stat_partial, N, H, W, C, stride, Ho, Wo);
    else hipLaunchKernelGGL((dw_fwd_kernel<CLc, 5>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, x, w, y, stat_partial, N, H, W, C, stride, Ho, Wo);
  });
  LMKD_CHECK_LAUNCH("dw_fwd_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_dw_conv_bwd_data(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int stride, void* stream) {
  const char* e = dw_check(N, H, W, C, K, stride);
  LMKD_REQUIRE(!e, "lmkd_dw_conv_bwd_data: %s (N=%d H=%d W=%d C=%d K=%d stride=%d)", e ? e : "", N, H, W, C, K, stride);
  LMKD_REQUIRE(dy && w && dx && aligned16(dy) && aligned16(dx), "lmkd_dw_conv_bwd_data: null or unaligned pointer");
  const int Ho = dw_out(H, K, stride), Wo = dw_out(W, K, stride), CL = mn_cl(C);
  const long npix = (long)N * H * W;
  const long blocks = std::min<long>((npix + (MN_THREADS / CL) - 1) / (MN_THREADS / CL), 4096);
  const dim3 grid((unsigned)blocks, C / (4 * CL));
  MN_DISPATCH_CL(CL, {
    if (K == 3) hipLaunchKernelGGL((dw_dgrad_kernel<CLc, 3>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, dy, w, dx, npix, H, W, C, stride, Ho, Wo);
    else hipLaunchKernelGGL((dw_dgrad_kernel<CLc, 5>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, dy, w, dx, npix, H, W, C, stride, Ho, Wo);
  });
  LMKD_CHECK_LAUNCH("dw_dgrad_kernel");
  return LMKD_OK;
}

extern "C" long lmkd_dw_conv_bwd_weight_workspace(int N, int H, int W, int C, int K, int stride) {
  if (dw_check(N, H, W, C, K, stride)) return 0;
  return red_tiles((long)N * dw_out(H, K, stride) * dw_out(W, K, stride)) * C * K * K * (long)sizeof(float);
}

extern "C" int lmkd_dw_conv_bwd_weight(const float* x, const float* dy, float* dw, void* workspace, long ws_bytes, int N, int H, int W, int C,
                                       int K, int stride, int accumulate, void* stream) {
  const char* e = dw_check(N, H, W, C, K, stride);
  LMKD_REQUIRE(!e, "lmkd_dw_conv_bwd_weight: %s (N=%d H=%d W=%d C=%d K=%d stride=%d)", e ? e : "", N, H, W, C, K, stride);
  LMKD_REQUIRE(x && dy && dw && workspace && aligned16(x) && aligned16(dy), "lmkd_dw_conv_bwd_weight: null or unaligned pointer");
  LMKD_REQUIRE(ws_bytes >= lmkd_dw_conv_bwd_weight_workspace(N, H, W, C, K, stride), "lmkd_dw_conv_bwd_weight: workspace too small");
  const int Ho = dw_out(H, K, stride), Wo = dw_out(W, K, stride), CL = mn_cl(C);
  const long T = red_tiles((long)N * Ho * Wo);
  const dim3 grid((unsigned)T, C / (4 * CL));
  float* part = (float*)workspace;
  MN_DISPATCH_CL(CL, {
    if (K == 3) hipLaunchKernelGGL((dw_wgrad_kernel<CLc, 3>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, x, dy, part, N, H, W, C, stride, Ho, Wo);
    else hipLaunchKernelGGL((dw_wgrad_kernel<CLc, 5>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, x, dy, part, N, H, W, C, stride, Ho, Wo);
  });
  LMKD_CHECK_LAUNCH("dw_wgrad_kernel");
  return col_reduce(part, T, (long)C * K * K, dw, accumulate, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------
// column statistics of a [rows][C] tensor (the output of a 1 x 1 convolution GEMM): part[tile][C][2] = (sum, sum of squares) over the
// tile's MN_TILE_STAT rows - the partial-sum buffer of lmkd_bn_finalize
// ---------------------------------------------------------------------------------
template <int CL>
__global__ void __launch_bounds__(MN_THREADS) col_stats_kernel(const float* __restrict__ x, float* __restrict__ part, long rows, int C) {
  constexpr int PL = MN_THREADS / CL;
  __shared__ float red[2 * MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  const long p0 = (long)blockIdx.x * MN_TILE_STAT;
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  for (int i = pl; i < MN_TILE_STAT; i += PL) {
    const long p = p0 + i;
    if (p >= rows) break;
    const float4 v = ld4(x + p * C + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float o = f4get(v, q); acc[0][q] += o; acc[1][q] += o * o; }
  }
  float* pt = part + (long)blockIdx.x * C * 2 + (long)blockIdx.y * 4 * CL * 2;
  lane_reduce<CL, 2>(acc, red, [&](int k, int cc, float s) { pt[cc * 2 + k] = s; });
}

extern "C" int lmkd_col_stats(const float* x, float* stat_partial, long rows, int C, void* stream) {
  LMKD_REQUIRE(x && stat_partial && aligned16(x) && rows > 0 && C > 0 && C % 8 == 0, "lmkd_col_stats: bad arguments (rows=%ld C=%d)", rows, C);
  const int CL = mn_cl(C);
  const dim3 grid((unsigned)lmkd_mnv3_stat_tiles(rows), C / (4 * CL));
  MN_DISPATCH_CL(CL, hipLaunchKernelGGL((col_stats_kernel<CLc>), grid, dim3(MN_THREADS), 0, (hipStream_t)stream, x, stat_partial, rows, C));
  LMKD_CHECK_LAUNCH("col_stats_kernel");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// BatchNorm apply + activation (+ residual): y = act(x scale + shift) (+ res).  stats: the [5][C] table of lmkd_bn_finalize (train) or
// lmkd_bn_eval_stats (eval).  16 bytes per lane, grid-stride.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(MN_THREADS) bn_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                                const float* __restrict__ res, float* __restrict__ y, long n4, int C, int act) {
  const float* scale = stats + 2 * C;
  const float* shift = stats + 3 * C;
  for (long i = (long)blockIdx.x * MN_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * MN_THREADS) {
    const int c = (int)((i * 4) % C);
    const float4 v = ld4(x + i * 4);
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = act_fwd(f4get(v, q) * scale[c + q] + shift[c + q], act);
    if (res) {
      const float4 r = ld4(res + i * 4);
      o[0] += r.x; o[1] += r.y; o[2] += r.z; o[3] += r.w;
    }
    st4(y + i * 4, make_float4(o[0], o[1], o[2], o[3]));
  }
}

static inline unsigned mn_ew_grid(long n4) { return (unsigned)std::max<long>(1, std::min<long>((n4 + MN_THREADS - 1) / MN_THREADS, 2048)); }

extern "C" int lmkd_bn_act_fwd(const float* x, const float* stats, const float* res, float* y, long rows, int C, int act, void* stream) {
  LMKD_REQUIRE(x && stats && y && rows > 0 && C > 0 && C % 8 == 0 && act >= 0 && act <= 2, "lmkd_bn_act_fwd: bad arguments (rows=%ld C=%d act=%d)",
               rows, C, act);
  LMKD_REQUIRE(aligned16(x) && aligned16(y) && (!res || aligned16(res)), "lmkd_bn_act_fwd: unaligned tensor");
  const long n4 = rows * C / 4;
  hipLaunchKernelGGL(bn_act_fwd_kernel, dim3(mn_ew_grid(n4)), dim3(MN_THREADS), 0, (hipStream_t)stream, x, stats, res, y, n4, C, act);
  LMKD_CHECK_LAUNCH("bn_act_fwd_kernel");
  return LMKD_OK;
}

// train-mode backward, pass 1: per tile, sum g and sum g xhat with g = dy act'(x scale + shift) (the activation's derivative recomputed from
// the BatchNorm input and the stats table: no mask tensor) -> part[tile][2][C], in double: these sums are exactly zero for every BatchNorm
// whose output reaches only train-mode BatchNorms through linear layers (most project BatchNorms), and an fp32 running sum over a lane's
// pixels would leave a residue well above the rounding of the gradient itself
template <int CL>
__global__ void __launch_bounds__(MN_THREADS) bn_act_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                       const float* __restrict__ stats, double* __restrict__ part, long rows, int C,
                                                                       int act) {
  constexpr int PL = MN_THREADS / CL;
  __shared__ double red[2 * MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  float mean[4], invstd[4], scale[4], shift[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    mean[q] = stats[c0 + q]; invstd[q] = stats[C + c0 + q]; scale[q] = stats[2 * C + c0 + q]; shift[q] = stats[3 * C + c0 + q];
  }
  const long p0 = (long)blockIdx.x * MN_TILE_RED;
  double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  for (int i = pl; i < MN_TILE_RED; i += PL) {
    const long p = p0 + i;
    if (p >= rows) break;
    const float4 v = ld4(x + p * C + c0), d = ld4(dy + p * C + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float xv = f4get(v, q);
      const float g = act_bwd(xv * scale[q] + shift[q], f4get(d, q), act);
      acc[0][q] += (double)g;
      acc[1][q] += (double)(g * ((xv - mean[q]) * invstd[q]));
    }
  }
  double* pt = part + (long)blockIdx.x * 2 * C + (long)blockIdx.y * 4 * CL;
  lane_reduce<CL, 2>(acc, red, [&](int k, int cc, double s) { pt[k * C + cc] = s; });
}

// pass 3: dx = gamma invstd (g - sum g / n - xhat sum g xhat / n)   (torch's batch_norm_backward, train mode)
__global__ void __launch_bounds__(MN_THREADS) bn_act_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                      const float* __restrict__ sums, float* __restrict__ dx, long n4, int C,
                                                                      float inv_count, int act) {
  for (long i = (long)blockIdx.x * MN_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * MN_THREADS) {
    const int c = (int)((i * 4) % C);
    const float4 v = ld4(x + i * 4), d = ld4(dy + i * 4);
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cc = c + q;
      const float xv = f4get(v, q);
      const float mean = stats[cc], invstd = stats[C + cc];
      const float g = act_bwd(xv * stats[2 * C + cc] + stats[3 * C + cc], f4get(d, q), act);
      const float gm = sums[cc] * inv_count, gx = sums[C + cc] * inv_count;
      const float xhat = (xv - mean) * invstd;
      o[q] = (g - gm - xhat * gx) * invstd * (gamma ? gamma[cc] : 1.f);
    }
    st4(dx + i * 4, make_float4(o[0], o[1], o[2], o[3]));
  }
}

extern "C" long lmkd_bn_act_bwd_workspace(long rows, int C) { return rows > 0 && C > 0 ? red_tiles(rows) * 2 * C * (long)sizeof(double) : 0; }

extern "C" int lmkd_bn_act_bwd(const float* dy, const float* x, const float* stats, const float* gamma, float* dx, float* dparams, void* workspace,
                               long ws_bytes, long rows, int C, int act, void* stream) {
  LMKD_REQUIRE(dy && x && stats && dx && dparams && workspace && rows > 0 && C > 0 && C % 8 == 0 && act >= 0 && act <= 2,
               "lmkd_bn_act_bwd: bad arguments (rows=%ld C=%d act=%d)", rows, C, act);
  LMKD_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(dx), "lmkd_bn_act_bwd: unaligned tensor");
  LMKD_REQUIRE(ws_bytes >= lmkd_bn_act_bwd_workspace(rows, C), "lmkd_bn_act_bwd: workspace too small");
  const int CL = mn_cl(C);
  const long T = red_tiles(rows);
  double* part = (double*)workspace;
  MN_DISPATCH_CL(CL, hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<CLc>), dim3((unsigned)T, C / (4 * CL)), dim3(MN_THREADS), 0, (hipStream_t)stream,
                                         dy, x, stats, part, rows, C, act));
  LMKD_CHECK_LAUNCH("bn_act_bwd_reduce_kernel");
  int rc = col_reduce(part, T, 2L * C, dparams, 0, (hipStream_t)stream);      // dparams = [sum g (= dbeta)][sum g xhat (= dgamma)]
  if (rc) return rc;
  const long n4 = rows * C / 4;
  hipLaunchKernelGGL(bn_act_bwd_apply_kernel, dim3(mn_ew_grid(n4)), dim3(MN_THREADS), 0, (hipStream_t)stream, dy, x, stats, gamma, dparams, dx, n4, C,
                     (float)(1.0 / (double)rows), act);
  LMKD_CHECK_LAUNCH("bn_act_bwd_apply_kernel");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// squeeze-excitation (torchvision SqueezeExcitation): m[n][c] = mean over H W of a; y = a s[n][c]; the backward's ds[n][c] = sum dy a and
// da = dy s (+ dm[n][c] / HW, the mean's gradient once the fc chain has produced it).  One workgroup per (frame, channel group).
// ---------------------------------------------------------------------------------
template <int CL>
__global__ void __launch_bounds__(MN_THREADS) se_mean_kernel(const float* __restrict__ a, float* __restrict__ m, int HW, int C) {
  constexpr int PL = MN_THREADS / CL;
  __shared__ float red[MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  const long n = blockIdx.x;
  float acc[1][4] = {{0.f, 0.f, 0.f, 0.f}};
  for (int p = pl; p < HW; p += PL) {
    const float4 v = ld4(a + (n * HW + p) * C + c0);
    acc[0][0] += v.x; acc[0][1] += v.y; acc[0][2] += v.z; acc[0][3] += v.w;
  }
  float* mo = m + n * C + blockIdx.y * 4 * CL;
  const float inv = 1.f / (float)HW;
  lane_reduce<CL, 1>(acc, red, [&](int, int cc, float s) { mo[cc] = s * inv; });
}

template <int CL>
__global__ void __launch_bounds__(MN_THREADS) se_scale_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a, const float* __restrict__ s,
                                                                  const float* __restrict__ dm, float* __restrict__ da, float* __restrict__ ds, int HW,
                                                                  int C) {
  constexpr int PL = MN_THREADS / CL;
  __shared__ float red[MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int c0 = blockIdx.y * 4 * CL + cl * 4;
  const long n = blockIdx.x;
  float sv[4], mv[4];
  const float inv = 1.f / (float)HW;
#pragma unroll
  for (int q = 0; q < 4; ++q) { sv[q] = s[n * C + c0 + q]; mv[q] = dm ? dm[n * C + c0 + q] * inv : 0.f; }
  float acc[1][4] = {{0.f, 0.f, 0.f, 0.f}};
  for (int p = pl; p < HW; p += PL) {
    const long o = (n * HW + p) * C + c0;
    const float4 g = ld4(dy + o);
    if (ds) {
      const float4 v = ld4(a + o);
      acc[0][0] += g.x * v.x; acc[0][1] += g.y * v.y; acc[0][2] += g.z * v.z; acc[0][3] += g.w * v.w;
    }
    if (da) st4(da + o, make_float4(g.x * sv[0] + mv[0], g.y * sv[1] + mv[1], g.z * sv[2] + mv[2], g.w * sv[3] + mv[3]));
  }
  if (!ds) return;      // uniform
  float* so = ds + n * C + blockIdx.y * 4 * CL;
  lane_reduce<CL, 1>(acc, red, [&](int, int cc, float v) { so[cc] = v; });
}

__global__ void __launch_bounds__(MN_THREADS) se_scale_fwd_kernel(const float* __restrict__ a, const float* __restrict__ s, float* __restrict__ y,
                                                                  long n4, long hwc, int C) {
  for (long i = (long)blockIdx.x * MN_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * MN_THREADS) {
    const long e = i * 4;
    const long n = e / hwc;
    const int c = (int)(e % C);
    const float4 v = ld4(a + e);
    const float* sp = s + n * C + c;
    st4(y + e, make_float4(v.x * sp[0], v.y * sp[1], v.z * sp[2], v.w * sp[3]));
  }
}

__global__ void hardsigmoid_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * MN_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * MN_THREADS) {
    const float v = x[i];
    if (dy) y[i] = (v > -3.f && v < 3.f) ? dy[i] / 6.f : 0.f;
    else y[i] = fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f;
  }
}

static const char* se_check(const float* a, int N, int HW, int C) {
  if (!a || N <= 0 || HW <= 0 || C <= 0) return "bad arguments";
  if (C % 8) return "C % 8 != 0";
  if (!aligned16(a)) return "unaligned tensor";
  return nullptr;
}

extern "C" int lmkd_se_mean(const float* a, float* m, int N, int HW, int C, void* stream) {
  const char* e = se_check(a, N, HW, C);
  LMKD_REQUIRE(!e && m, "lmkd_se_mean: %s (N=%d HW=%d C=%d)", e ? e : "null output", N, HW, C);
  const int CL = mn_cl(C);
  MN_DISPATCH_CL(CL, hipLaunchKernelGGL((se_mean_kernel<CLc>), dim3(N, C / (4 * CL)), dim3(MN_THREADS), 0, (hipStream_t)stream, a, m, HW, C));
  LMKD_CHECK_LAUNCH("se_mean_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_se_scale_fwd(const float* a, const float* s, float* y, int N, int HW, int C, void* stream) {
  const char* e = se_check(a, N, HW, C);
  LMKD_REQUIRE(!e && s && y && aligned16(y), "lmkd_se_scale_fwd: %s (N=%d HW=%d C=%d)", e ? e : "null / unaligned output", N, HW, C);
  const long n4 = (long)N * HW * C / 4;
  hipLaunchKernelGGL(se_scale_fwd_kernel, dim3(mn_ew_grid(n4)), dim3(MN_THREADS), 0, (hipStream_t)stream, a, s, y, n4, (long)HW * C, C);
  LMKD_CHECK_LAUNCH("se_scale_fwd_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_se_scale_bwd(const float* dy, const float* a, const float* s, const float* dm, float* da, float* ds, int N, int HW, int C,
                                 void* stream) {
  const char* e = se_check(dy, N, HW, C);
  LMKD_REQUIRE(!e && s && (da || ds), "lmkd_se_scale_bwd: %s (N=%d HW=%d C=%d)", e ? e : "nothing to compute", N, HW, C);
  LMKD_REQUIRE(!ds || (a && aligned16(a)), "lmkd_se_scale_bwd: ds needs the scaled tensor a");
  LMKD_REQUIRE(!da || aligned16(da), "lmkd_se_scale_bwd: unaligned da");
  const int CL = mn_cl(C);
  MN_DISPATCH_CL(CL, hipLaunchKernelGGL((se_scale_bwd_kernel<CLc>), dim3(N, C / (4 * CL)), dim3(MN_THREADS), 0, (hipStream_t)stream, dy, a, s, dm, da,
                                         ds, HW, C));
  LMKD_CHECK_LAUNCH("se_scale_bwd_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_hardsigmoid_fwd(const float* x, float* y, long n, void* stream) {
  LMKD_REQUIRE(x && y && n > 0, "lmkd_hardsigmoid_fwd: bad arguments");
  hipLaunchKernelGGL(hardsigmoid_kernel, dim3(mn_ew_grid(n / 4 + 1)), dim3(MN_THREADS), 0, (hipStream_t)stream, x, (const float*)nullptr, y, n);
  LMKD_CHECK_LAUNCH("hardsigmoid_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_hardsigmoid_bwd(const float* dy, const float* x, float* dx, long n, void* stream) {
  LMKD_REQUIRE(dy && x && dx && n > 0, "lmkd_hardsigmoid_bwd: bad arguments");
  hipLaunchKernelGGL(hardsigmoid_kernel, dim3(mn_ew_grid(n / 4 + 1)), dim3(MN_THREADS), 0, (hipStream_t)stream, x, dy, dx, n);
  LMKD_CHECK_LAUNCH("hardsigmoid_kernel");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// stem: Conv 3 -> 16, 3 x 3, stride 2, pad 1 on the NHWC4 input (channel 3 is the zero pad of lmkd_frames_*_nhwc4 / lmkd_nchw3_to_nhwc4).
// w: [16][3][3][3] (OIHW).  Forward: one output pixel x 4 output channels per lane (CL = 4), the lane's 4 x 27 weights in registers,
// BatchNorm partial sums in part[tile][16][2].  Weight gradient: per-tile sums of the 4 x 27 products -> part[tile][16 * 27] (OIHW order),
// col_reduce_kernel over the tiles.
// ---------------------------------------------------------------------------------
#define STEM_CO 16
template <bool WGRAD>
__global__ void __launch_bounds__(MN_THREADS) stem3_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy,
                                                           float* __restrict__ y, float* __restrict__ part, int N, int H, int W, int Ho, int Wo) {
  constexpr int CL = 4, PL = MN_THREADS / CL, TILE = WGRAD ? MN_TILE_RED : MN_TILE_STAT;
  __shared__ float red[(WGRAD ? 8 : 2) * MN_THREADS * 4];
  const int tid = threadIdx.x, cl = tid % CL, pl = tid / CL;
  const int o0 = cl * 4;
  float wr[27][4];      // forward: weights; weight gradient: accumulators
#pragma unroll
  for (int j = 0; j < 27; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) wr[j][q] = WGRAD ? 0.f : w[(o0 + q) * 27 + j];
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const long npix = (long)N * Ho * Wo;
  const long p0 = (long)blockIdx.x * TILE;
  for (int i = pl; i < TILE; i += PL) {
    const long p = p0 + i;
    if (p >= npix) break;
    const int ow = (int)(p % Wo);
    const long r = p / Wo;
    const int oh = (int)(r % Ho);
    const long n = r / Ho;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (WGRAD) g = ld4(dy + p * STEM_CO + o0);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh * 2 - 1 + kh;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = ow * 2 - 1 + kw;
        if (iw < 0 || iw >= W) continue;
        const float4 v = ld4(x + ((n * H + ih) * W + iw) * 4);
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float xv = ci == 0 ? v.x : (ci == 1 ? v.y : v.z);
          const int j = ci * 9 + kh * 3 + kw;
          if (WGRAD) {
            wr[j][0] += g.x * xv; wr[j][1] += g.y * xv; wr[j][2] += g.z * xv; wr[j][3] += g.w * xv;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] += xv * wr[j][q];
          }
        }
      }
    }
    if (!WGRAD) {
      st4(y + p * STEM_CO + o0, make_float4(o[0], o[1], o[2], o[3]));
#pragma unroll
      for (int q = 0; q < 4; ++q) { acc[0][q] += o[q]; acc[1][q] += o[q] * o[q]; }
    }
  }
  if (!WGRAD) {
    if (!part) return;
    float* pt = part + (long)blockIdx.x * STEM_CO * 2;
    lane_reduce<CL, 2>(acc, red, [&](int k, int cc, float s) { pt[cc * 2 + k] = s; });
    return;
  }
  float* pt = part + (long)blockIdx.x * STEM_CO * 27;
#pragma unroll
  for (int j0 = 0; j0 < 27; j0 += 8) {
    const int nt = 27 - j0 < 8 ? 27 - j0 : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(j * PL + pl) * (4 * CL) + cl * 4 + q] = wr[j0 + j < 27 ? j0 + j : 0][q];
    __syncthreads();
    for (int col = tid; col < nt * 4 * CL; col += MN_THREADS) {
      const int j = col / (4 * CL), cc = col % (4 * CL);
      float s = 0.f;
      for (int pp = 0; pp < PL; ++pp) s += red[(j * PL + pp) * (4 * CL) + cc];
      pt[cc * 27 + j0 + j] = s;
    }
    __syncthreads();
  }
}

static inline int stem_out(int H) { return (H - 1) / 2 + 1; }      // (H + 2 - 3) / 2 + 1

extern "C" int lmkd_stem3x3_fwd(const float* x4, const float* w, float* y, float* stat_partial, int N, int H, int W, void* stream) {
  LMKD_REQUIRE(x4 && w && y && N > 0 && H > 0 && W > 0 && aligned16(x4) && aligned16(y), "lmkd_stem3x3_fwd: bad arguments");
  const int Ho = stem_out(H), Wo = stem_out(W);
  hipLaunchKernelGGL(stem3_kernel<false>, dim3((unsigned)lmkd_mnv3_stat_tiles((long)N * Ho * Wo)), dim3(MN_THREADS), 0, (hipStream_t)stream, x4, w,
                     (const float*)nullptr, y, stat_partial, N, H, W, Ho, Wo);
  LMKD_CHECK_LAUNCH("stem3_kernel");
  return LMKD_OK;
}

extern "C" long lmkd_stem3x3_bwd_weight_workspace(int N, int H, int W) {
  return N > 0 && H > 0 && W > 0 ? red_tiles((long)N * stem_out(H) * stem_out(W)) * STEM_CO * 27 * (long)sizeof(float) : 0;
}

extern "C" int lmkd_stem3x3_bwd_weight(const float* x4, const float* dy, float* dw, void* workspace, long ws_bytes, int N, int H, int W, int accumulate,
                                       void* stream) {
  LMKD_REQUIRE(x4 && dy && dw && workspace && N > 0 && H > 0 && W > 0 && aligned16(x4) && aligned16(dy), "lmkd_stem3x3_bwd_weight: bad arguments");
  LMKD_REQUIRE(ws_bytes >= lmkd_stem3x3_bwd_weight_workspace(N, H, W), "lmkd_stem3x3_bwd_weight: workspace too small");
  const int Ho = stem_out(H), Wo = stem_out(W);
  const long T = red_tiles((long)N * Ho * Wo);
  hipLaunchKernelGGL(stem3_kernel<true>, dim3((unsigned)T), dim3(MN_THREADS), 0, (hipStream_t)stream, x4, (const float*)nullptr, dy, (float*)nullptr,
                     (float*)workspace, N, H, W, Ho, Wo);
  LMKD_CHECK_LAUNCH("stem3_kernel");
  return col_reduce((const float*)workspace, T, STEM_CO * 27, dw, accumulate, (hipStream_t)stream);
}
