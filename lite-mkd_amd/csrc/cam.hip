// Attention maps of the students (reference: heatmap_vis.py:20-48, teacher/code/heatmap_vis.py:16-27 - Grad-CAM on the last trunk
// stage, the map laid over the frame).  Two kernels:
//   lmkd_gradcam_fwd     the map entering the pooled head and its gradient -> channel weights, the ReLU'd map, the min-max normalised map
//   lmkd_cam_overlay_u8  normalised map -> 8 bit -> Pillow's bilinear upsampling -> colour table -> blend with the RGB frame
// Both are deterministic: fixed-order reductions, no atomics, integer arithmetic after the quantisation.
#include "common.h"

// ---------------------------------------------------------------------------------
// Grad-CAM / HiResCAM.  One workgroup of 16 waves per frame.  The frame's [HW][C] map is walked as float4 columns: a wave owns 64
// adjacent float4 columns (wave j of the WPR = ceil(C / 256) waves that span a row) of the rows s, s + R, s + 2R, ... (R = 16 / WPR row
// slices), so a thread keeps ONE float4 column for the whole kernel:
//   column sums of dA   per-thread float4 over its rows, the R slices added in slice order through LDS -> w[c] = sum / HW, kept in LDS
//   raw[p]              per-thread 4-term dot, butterfly over the wave, the WPR wave values of a row added in wave order through LDS
//   min / max over p    per-thread over LDS raw, butterfly, 16 wave values in wave order
// mode 0 reads dA once (column sums) and then A once (dots with w); mode 1 reads A and dA together once (the column sums for the
// `weights` output ride along).  Rows are loaded four at a time per thread before the first reduction, so 4 (8) float4 loads are in
// flight per lane.
// ---------------------------------------------------------------------------------
#define CAM_THREADS 1024
#define CAM_WAVES (CAM_THREADS / 64)
#define CAM_MAX_C 4096                       // CAM_THREADS float4 columns
#define CAM_MAX_HW 2048                      // raw[] in LDS
#define CAM_ROWPART 4096                     // floats: wave values of one chunk of rows (the column-sum partials use the same words)
#define CAM_UNROLL 4

__device__ __forceinline__ float cam_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float cam_dot4(const float4& a, const float4& b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

// the R row slices' column sums, added in slice order -> w[c] = sum / HW in s_w (and in `weights`); every thread of the workgroup calls it
__device__ __forceinline__ void cam_finish_colsum(const float4 acc, float4* __restrict__ part4, float4* __restrict__ s_w,
                                                  float* __restrict__ weights, bool on, int s, int col, int C4, int R, int HW) {
  const int tid = threadIdx.x;
  if (on) part4[s * C4 + col] = acc;
  __syncthreads();
  if (tid < C4) {
    float4 t = part4[tid];
    for (int r = 1; r < R; ++r) {
      const float4 u = part4[r * C4 + tid];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    const float n = (float)HW;
    t.x /= n; t.y /= n; t.z /= n; t.w /= n;
    s_w[tid] = t;
    if (weights) reinterpret_cast<float4*>(weights)[tid] = t;
  }
  __syncthreads();
}

template <int MODE>
__global__ void __launch_bounds__(CAM_THREADS)
gradcam_kernel(const float* __restrict__ A, const float* __restrict__ dA, float* __restrict__ weights, float* __restrict__ raw_out,
               float* __restrict__ cam_out, int HW, int C) {
  __shared__ float4 s_w[CAM_THREADS];            // w[c], float4 column k at s_w[k]
  __shared__ __attribute__((aligned(16))) float s_part[CAM_ROWPART];          // column-sum partials [R][C4] float4, then the rows' wave values [rows of a chunk][WPR]
  __shared__ float s_raw[CAM_MAX_HW];
  __shared__ float s_mn[CAM_WAVES], s_mx[CAM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int C4 = C >> 2;
  const int WPR = (C4 + 63) >> 6;                // waves that span a row (1..16)
  const int R = CAM_WAVES / WPR;                 // row slices
  const int s = wv / WPR, j = wv - s * WPR;
  const int col = j * 64 + lane;
  const bool wave_on = s < R;
  const bool on = wave_on && col < C4;
  const size_t base = (size_t)blockIdx.x * HW * C;
  const float4* __restrict__ A4 = reinterpret_cast<const float4*>(A + base) + (on ? col : 0);
  const float4* __restrict__ D4 = reinterpret_cast<const float4*>(dA + base) + (on ? col : 0);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float* __restrict__ wout = weights ? weights + (size_t)blockIdx.x * C : nullptr;
  float4 acc = zero4;                            // column sums of dA over this thread's rows

  if (MODE == 0) {
    if (on) {
      for (int p0 = s; p0 < HW; p0 += R * CAM_UNROLL) {
        float4 d[CAM_UNROLL];
#pragma unroll
        for (int u = 0; u < CAM_UNROLL; ++u) {
          const int p = p0 + u * R;
          d[u] = zero4;
          if (p < HW) d[u] = D4[(size_t)p * C4];
        }
#pragma unroll
        for (int u = 0; u < CAM_UNROLL; ++u) { acc.x += d[u].x; acc.y += d[u].y; acc.z += d[u].z; acc.w += d[u].w; }
      }
    }
    cam_finish_colsum(acc, reinterpret_cast<float4*>(s_part), s_w, wout, on, s, col, C4, R, HW);
  }
  float4 w4 = zero4;
  if (MODE == 0 && on) w4 = s_w[col];

  // raw[p], a chunk of rows at a time (one chunk unless HW * WPR > CAM_ROWPART)
  const int chunk = CAM_ROWPART / WPR;
  for (int c0 = 0; c0 < HW; c0 += chunk) {
    const int c1 = min(HW, c0 + chunk);
    if (wave_on) {
      for (int p0 = c0 + s; p0 < c1; p0 += R * CAM_UNROLL) {
        float4 a[CAM_UNROLL], d[CAM_UNROLL];
#pragma unroll
        for (int u = 0; u < CAM_UNROLL; ++u) {
          const int p = p0 + u * R;
          const bool ld = on && p < c1;
          a[u] = zero4;
          d[u] = zero4;
          if (ld) a[u] = A4[(size_t)p * C4];
          if (MODE == 1 && ld) d[u] = D4[(size_t)p * C4];
        }
#pragma unroll
        for (int u = 0; u < CAM_UNROLL; ++u) {
          const int p = p0 + u * R;
          float v;
          if (MODE == 1) {
            v = cam_dot4(d[u], a[u]);
            acc.x += d[u].x; acc.y += d[u].y; acc.z += d[u].z; acc.w += d[u].w;
          } else {
            v = cam_dot4(w4, a[u]);
          }
          v = cam_wave_sum(v);
          if (lane == 0 && p < c1) s_part[(p - c0) * WPR + j] = v;
        }
      }
    }
    __syncthreads();
    for (int p = c0 + tid; p < c1; p += CAM_THREADS) {
      float v = s_part[(p - c0) * WPR];
      for (int k = 1; k < WPR; ++k) v += s_part[(p - c0) * WPR + k];
      s_raw[p] = fmaxf(v, 0.f);
    }
    __syncthreads();
  }
  if (MODE == 1 && weights) cam_finish_colsum(acc, reinterpret_cast<float4*>(s_part), s_w, wout, on, s, col, C4, R, HW);     // (uniform: `weights` is a kernel argument)

  // min / max over the frame's positions, then the normalised map
  float mn = 3.402823466e38f, mx = 0.f;          // raw >= 0
  for (int p = tid; p < HW; p += CAM_THREADS) {
    const float v = s_raw[p];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) { s_mn[wv] = mn; s_mx[wv] = mx; }
  __syncthreads();
  mn = s_mn[0]; mx = s_mx[0];
  for (int k = 1; k < CAM_WAVES; ++k) { mn = fminf(mn, s_mn[k]); mx = fmaxf(mx, s_mx[k]); }
  const float den = 1e-7f + (mx - mn);            // (the range first: added to mx, 1e-7 is lost in fp32 and a constant map would divide 0 by 0)
  for (int p = tid; p < HW; p += CAM_THREADS) {
    const float v = s_raw[p];
    raw_out[(size_t)blockIdx.x * HW + p] = v;
    cam_out[(size_t)blockIdx.x * HW + p] = (v - mn) / den;
  }
}

extern "C" int lmkd_gradcam_fwd(const float* A, const float* dA, float* weights, float* raw, float* cam, int F, int HW, int C, int mode,
                                void* stream) {
  LMKD_REQUIRE(mode == 0 || mode == 1, "lmkd_gradcam_fwd: mode %d (0 = Grad-CAM, 1 = HiResCAM)", mode);
  LMKD_REQUIRE(C >= 8 && C % 8 == 0 && C <= CAM_MAX_C, "lmkd_gradcam_fwd: C %d must be a multiple of 8 in 8..%d", C, CAM_MAX_C);
  LMKD_REQUIRE(HW >= 1 && HW <= CAM_MAX_HW, "lmkd_gradcam_fwd: HW %d outside 1..%d", HW, CAM_MAX_HW);
  LMKD_REQUIRE(F >= 1, "lmkd_gradcam_fwd: F %d must be positive", F);
  LMKD_REQUIRE(A && dA && raw && cam, "lmkd_gradcam_fwd: null A / dA / raw / cam");
  LMKD_REQUIRE(aligned16(A) && aligned16(dA) && (!weights || aligned16(weights)), "lmkd_gradcam_fwd: A / dA / weights must be 16-byte aligned");
  if (mode == 0)
    hipLaunchKernelGGL(gradcam_kernel<0>, dim3(F), dim3(CAM_THREADS), 0, (hipStream_t)stream, A, dA, weights, raw, cam, HW, C);
  else
    hipLaunchKernelGGL(gradcam_kernel<1>, dim3(F), dim3(CAM_THREADS), 0, (hipStream_t)stream, A, dA, weights, raw, cam, HW, C);
  LMKD_CHECK_LAUNCH("gradcam_kernel");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// The overlay.  A thread owns one output pixel: q = min(255, (int)(cam * 255 + 0.5f)) of the (at most ksize_v x ksize_h) map positions
// it needs, Pillow's horizontal pass at its own column for each of those rows (rounded and clipped to uint8 as Pillow's intermediate
// image is), the vertical pass over them, the colour of the resulting byte, the blend.  Integers from the quantisation on.
// ---------------------------------------------------------------------------------
#define CAM_PIL_PRECISION_BITS 22                // (Pillow's PRECISION_BITS = 32 - 8 - 2, as lmkd_resize_plan's tables)
#define CAM_OV_THREADS 256

__device__ __forceinline__ int cam_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ void __launch_bounds__(CAM_OV_THREADS)
cam_overlay_u8_kernel(const float* __restrict__ cam, const unsigned char* __restrict__ frames, unsigned char* __restrict__ out,
                      const int* __restrict__ bh, const int* __restrict__ kh, int ksh, const int* __restrict__ bv,
                      const int* __restrict__ kv, int ksv, const unsigned char* __restrict__ lut, int h, int w, int Ho, int Wo, int alpha) {
  const int f = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= Ho * Wo) return;
  const int oy = p / Wo, ox = p - oy * Wo;
  const int x0 = bh[ox * 2], nx = bh[ox * 2 + 1];
  const int y0 = bv[oy * 2], ny = bv[oy * 2 + 1];
  const int* ch = kh + (size_t)ox * ksh;
  const int* cv = kv + (size_t)oy * ksv;
  const float* m = cam + (size_t)f * h * w;
  int acc = 1 << (CAM_PIL_PRECISION_BITS - 1);
  for (int yy = 0; yy < ny; ++yy) {
    const float* row = m + (size_t)(y0 + yy) * w + x0;
    int t = 1 << (CAM_PIL_PRECISION_BITS - 1);
    for (int xx = 0; xx < nx; ++xx) {
      const int q = cam_clip8((int)(row[xx] * 255.f + 0.5f));
      t += q * ch[xx];
    }
    acc += cam_clip8(t >> CAM_PIL_PRECISION_BITS) * cv[yy];
  }
  const int v = cam_clip8(acc >> CAM_PIL_PRECISION_BITS);
  const size_t o = ((size_t)f * Ho * Wo + p) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = lut[v * 3 + k];
    out[o + k] = (unsigned char)(frames ? ((c * (256 - alpha) + (int)frames[o + k] * alpha + 128) >> 8) : c);
  }
}

extern "C" int lmkd_cam_overlay_u8(const float* cam, const unsigned char* frames, unsigned char* out, const int* bounds_h, const int* coeffs_h,
                                   int ksize_h, const int* bounds_v, const int* coeffs_v, int ksize_v, const unsigned char* lut, int F, int h,
                                   int w, int Ho, int Wo, int alpha256, void* stream) {
  LMKD_REQUIRE(alpha256 >= 0 && alpha256 <= 256, "lmkd_cam_overlay_u8: alpha256 %d outside 0..256", alpha256);
  LMKD_REQUIRE(F >= 1 && F <= 65535, "lmkd_cam_overlay_u8: F %d outside 1..65535", F);
  LMKD_REQUIRE(h >= 1 && w >= 1 && Ho >= 1 && Wo >= 1 && (long)Ho * Wo <= (1L << 30), "lmkd_cam_overlay_u8: bad sizes h %d w %d Ho %d Wo %d", h, w, Ho, Wo);
  LMKD_REQUIRE(ksize_h > 0 && ksize_v > 0, "lmkd_cam_overlay_u8: ksize_h %d / ksize_v %d must be positive", ksize_h, ksize_v);
  LMKD_REQUIRE(cam && out && bounds_h && coeffs_h && bounds_v && coeffs_v && lut, "lmkd_cam_overlay_u8: null cam / out / table / lut");
  hipLaunchKernelGGL(cam_overlay_u8_kernel, dim3(cdiv((long)Ho * Wo, CAM_OV_THREADS), F), dim3(CAM_OV_THREADS), 0, (hipStream_t)stream, cam,
                     frames, out, bounds_h, coeffs_h, ksize_h, bounds_v, coeffs_v, ksize_v, lut, h, w, Ho, Wo, alpha256);
  LMKD_CHECK_LAUNCH("cam_overlay_u8_kernel");
  return LMKD_OK;
}
