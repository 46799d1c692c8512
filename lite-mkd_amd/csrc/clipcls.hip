// The clip classifier the teacher's per-modality ResNet-50 is pretrained as (Action_Recognition_Resnet50): global average pool over
// the positions of a frame and over groups of consecutive frames, softmax cross-entropy over any number of classes, SGD with momentum
// over a flat buffer.  All three are HBM- or latency-bound; every sum runs in a fixed order (no atomics), so repeats are bit-identical.
#include "common.h"

#define CC_THREADS 256
#define CC_LANES 16      // lanes along C: 16 x 4 channels = 256 contiguous bytes of an fp32 row (128 of a bf16 row) per position
#define CC_SLOTS (CC_THREADS / CC_LANES)      // positions a workgroup reads side by side

// ---------------------------------------------------------------------------------
// global average pool: x [F, H*W, C] (NHWC, the trunk's storage type) -> y [F/G, C] fp32, the mean over the G*H*W positions of G
// consecutive frames.  A workgroup owns 64 channels of one output row: 16 lanes along C, 16 position slots; slot s sums the positions
// s, s + 16, ... in that order and slot 0 adds the 16 partial sums in slot order.  Grid (C / 64, F / G): 2048 workgroups for the
// extraction's [64, 49, 2048] at G = 1, 256 at G = 8.
// ---------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(CC_THREADS) global_avgpool_fwd_kernel(const T* __restrict__ x, float* __restrict__ y, int P, int C4) {
  __shared__ float4 part[CC_SLOTS][CC_LANES];
  const int lane = threadIdx.x & (CC_LANES - 1), slot = threadIdx.x / CC_LANES;
  const int c4 = blockIdx.x * CC_LANES + lane;
  const long n = blockIdx.y;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c4 < C4) {
    const long base = n * P * C4 + c4;
#pragma unroll 4
    for (int p = slot; p < P; p += CC_SLOTS) {
      const float4 v = ld4<T>(x, base + (long)p * C4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  part[slot][lane] = acc;
  __syncthreads();
  if (slot == 0 && c4 < C4) {
    float4 s = part[0][lane];
#pragma unroll
    for (int j = 1; j < CC_SLOTS; ++j) {
      const float4 v = part[j][lane];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float d = (float)P;
    reinterpret_cast<float4*>(y)[n * C4 + c4] = make_float4(s.x / d, s.y / d, s.z / d, s.w / d);
  }
}

// dx[f, p, c] = dy[f / G, c] / (G*H*W): the same workgroup shape, every slot writes its positions
template <typename T>
__global__ void __launch_bounds__(CC_THREADS) global_avgpool_bwd_kernel(const float* __restrict__ dy, T* __restrict__ dx, int P, int C4) {
  const int lane = threadIdx.x & (CC_LANES - 1), slot = threadIdx.x / CC_LANES;
  const int c4 = blockIdx.x * CC_LANES + lane;
  const long n = blockIdx.y;
  if (c4 >= C4) return;
  const float4 g = reinterpret_cast<const float4*>(dy)[n * C4 + c4];
  const float d = (float)P;
  const float4 v = make_float4(g.x / d, g.y / d, g.z / d, g.w / d);
  const long base = n * P * C4 + c4;
  for (int p = slot; p < P; p += CC_SLOTS) st4<T>(dx, base + (long)p * C4, v);
}

static int avgpool_check(const char* who, const void* a, const void* b, int F, int H, int W, int C, int G) {
  LMKD_REQUIRE(a && b, "%s: null pointer", who);
  LMKD_REQUIRE(F > 0 && H > 0 && W > 0 && C > 0 && G > 0, "%s: empty tensor (F=%d H=%d W=%d C=%d G=%d)", who, F, H, W, C, G);
  LMKD_REQUIRE(F % G == 0, "%s: %d frames are no multiple of the group of %d", who, F, G);
  LMKD_REQUIRE(C % 4 == 0, "%s: C=%d must be a multiple of 4", who, C);
  LMKD_REQUIRE(aligned16(a) && aligned16(b), "%s: tensors must be 16-byte aligned", who);
  LMKD_REQUIRE((long)G * H * W < 2147483647L && F / G <= 65535, "%s: %ld positions per group, %d groups: at most 2^31 - 1 and 65535", who,
               (long)G * H * W, F / G);
  return LMKD_OK;
}

extern "C" int lmkd_global_avgpool_fwd(const float* x, float* y, int F, int H, int W, int C, int G, void* stream) {
  if (int rc = avgpool_check("lmkd_global_avgpool_fwd", x, y, F, H, W, C, G)) return rc;
  const dim3 grid(cdiv(C / 4, CC_LANES), F / G);
  if (g_lmkd_act_bf16)
    hipLaunchKernelGGL(global_avgpool_fwd_kernel<lmkd_bf16_t>, grid, dim3(CC_THREADS), 0, (hipStream_t)stream, (const lmkd_bf16_t*)x, y, G * H * W, C / 4);
  else
    hipLaunchKernelGGL(global_avgpool_fwd_kernel<float>, grid, dim3(CC_THREADS), 0, (hipStream_t)stream, x, y, G * H * W, C / 4);
  LMKD_CHECK_LAUNCH("global_avgpool_fwd_kernel");
  return LMKD_OK;
}

extern "C" int lmkd_global_avgpool_bwd(const float* dy, float* dx, int F, int H, int W, int C, int G, void* stream) {
  if (int rc = avgpool_check("lmkd_global_avgpool_bwd", dy, dx, F, H, W, C, G)) return rc;
  const dim3 grid(cdiv(C / 4, CC_LANES), F / G);
  if (g_lmkd_act_bf16)
    hipLaunchKernelGGL(global_avgpool_bwd_kernel<lmkd_bf16_t>, grid, dim3(CC_THREADS), 0, (hipStream_t)stream, dy, (lmkd_bf16_t*)dx, G * H * W, C / 4);
  else
    hipLaunchKernelGGL(global_avgpool_bwd_kernel<float>, grid, dim3(CC_THREADS), 0, (hipStream_t)stream, dy, dx, G * H * W, C / 4);
  LMKD_CHECK_LAUNCH("global_avgpool_bwd_kernel");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// softmax cross-entropy (nn.CrossEntropyLoss, mean reduction) over [R, C] logits, any C >= 1: one wavefront per row, lane l takes the
// columns l, l + 64, ...; three passes over the row (maximum and first maximal index; sum of exp(s - max); gradient), the row being in
// cache after the first.  rows[2 r] = the row's loss, rows[2 r + 1] = 1 if its prediction equals its label; a second one-wavefront
// kernel sums them lane by lane in row order.  A label outside [0, C) is never used as an index: its row's loss is NaN.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) softmax_ce_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                     long long* __restrict__ pred, float* __restrict__ g,
                                                                     float* __restrict__ rows, int R, int C) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= R) return;      // wave-uniform
  const float* __restrict__ s = logits + (long)r * C;
  float m = -INFINITY;
  int am = lane < C ? lane : 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = s[c];
    if (v > m) { m = v; am = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) { m = om; am = oa; }
  }
  float z = 0.f;
  for (int c = lane; c < C; c += 64) z += expf(s[c] - m);
  z = wave_sum(z);
  const long long lab = labels[r];
  const bool ok = lab >= 0 && lab < C;
  if (g) {
    const float inv_r = 1.f / (float)R;
    for (int c = lane; c < C; c += 64) g[(long)r * C + c] = (expf(s[c] - m) / z - ((ok && c == (int)lab) ? 1.f : 0.f)) * inv_r;
  }
  if (lane == 0) {
    if (pred) pred[r] = am;
    rows[2 * r] = ok ? (m - s[lab]) + logf(z) : NAN;
    rows[2 * r + 1] = (ok && lab == am) ? 1.f : 0.f;
  }
}

__global__ void __launch_bounds__(64) softmax_ce_finish_kernel(const float* __restrict__ rows, float* __restrict__ out, int R) {
  float loss = 0.f, hit = 0.f;
  for (int r = threadIdx.x; r < R; r += 64) { loss += rows[2 * r]; hit += rows[2 * r + 1]; }
  loss = wave_sum(loss);
  hit = wave_sum(hit);
  if (threadIdx.x == 0) {
    out[0] = loss / (float)R;
    out[1] = hit / (float)R;
  }
}

// labels_host (nullable): the host copy of the labels, range-checked here before anything is launched
extern "C" int lmkd_softmax_ce(const float* logits, const long long* labels, const long long* labels_host, float* out2, long long* pred,
                               float* g, float* rows, int R, int C, void* stream) {
  LMKD_REQUIRE(R >= 1 && C >= 1, "lmkd_softmax_ce: %d rows of %d classes", R, C);
  LMKD_REQUIRE((long)R * C < 2147483647L, "lmkd_softmax_ce: %d x %d logits exceed 2^31 - 1", R, C);
  if (labels_host)
    for (int r = 0; r < R; ++r)
      LMKD_REQUIRE(labels_host[r] >= 0 && labels_host[r] < C, "lmkd_softmax_ce: label %lld of row %d outside [0, %d)", labels_host[r], r, C);
  LMKD_REQUIRE(logits && labels && out2 && rows, "lmkd_softmax_ce: null pointer");
  hipLaunchKernelGGL(softmax_ce_rows_kernel, dim3(cdiv(R, CC_THREADS / 64)), dim3(CC_THREADS), 0, (hipStream_t)stream, logits, labels, pred, g,
                     rows, R, C);
  hipLaunchKernelGGL(softmax_ce_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)rows, out2, R);
  LMKD_CHECK_LAUNCH("softmax_ce kernels");
  return LMKD_OK;
}

// ---------------------------------------------------------------------------------
// torch.optim.SGD(momentum, dampening 0, no Nesterov, no weight decay) over a flat buffer:
// buf = first ? g : momentum * buf + g;  p -= lr * buf;  g = 0 when asked
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(CC_THREADS) sgd_momentum_kernel(float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ buf, float lr,
                                                                  float mom, long n4, int first, int zero_grad) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 d = g[i];
    float4 b = d;
    if (!first) {
      const float4 o = buf[i];
      b = make_float4(mom * o.x + d.x, mom * o.y + d.y, mom * o.z + d.z, mom * o.w + d.w);
    }
    buf[i] = b;
    float4 w = p[i];
    w.x -= lr * b.x; w.y -= lr * b.y; w.z -= lr * b.z; w.w -= lr * b.w;
    p[i] = w;
    if (zero_grad) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
extern "C" int lmkd_sgd_momentum_step(float* param, float* grad, float* buf, float lr, float momentum, long n, int first, int zero_grad,
                                      void* stream) {
  LMKD_REQUIRE(param && grad && buf && n > 0 && n % 4 == 0 && aligned16(param) && aligned16(grad) && aligned16(buf),
               "lmkd_sgd_momentum_step: buffers must be 16-byte aligned, n %% 4 == 0");
  long gsz = (n / 4 + CC_THREADS - 1) / CC_THREADS;
  if (gsz > 2048) gsz = 2048;
  hipLaunchKernelGGL(sgd_momentum_kernel, dim3((unsigned)gsz), dim3(CC_THREADS), 0, (hipStream_t)stream, (float4*)param, (float4*)grad, (float4*)buf,
                     lr, momentum, n / 4, first, zero_grad);
  LMKD_CHECK_LAUNCH("sgd_momentum_kernel");
  return LMKD_OK;
}
