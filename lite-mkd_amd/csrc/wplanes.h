// The plane buffer of a convolution weight: its layout, its two fragment orders and its writers - stated HERE and nowhere else in csrc/.
// (DESIGN.md 3.1 shows the same table; tests/_wplanes_ref.py states it independently in numpy, and
// tests/test_gpu_ops.py test_weight_planes_match_the_layout_statement compares what the kernels below write with that statement bit for bit.)
//
// In every arithmetic except native fp32 the convolution kernels read the K-major packed weight Wp[col][Kp] (n = ncols * Kp elements,
// ncols and Kp multiples of 32) as 16-bit planes in MFMA fragment order.  In 16-bit elements:
//
//   mode 1 (bf16)   [0, n)                  one round-to-nearest bf16 plane, 32x32x16 order
//   modes 2 / 3     [0, 3n)                 the three truncation planes of W, 32x32x16 order     (X3FragB)
//                   [3n, 6n)                the same planes of -W
//                   [6n, 9n)                W, 16x16x32 order                                    (X3FragB16)
//                   [9n, 12n)               -W, 16x16x32 order
//   mode 4 adds     [12n, 14n)              the two fp16 planes of W 2^s, 16x16x32 order         (X3FragB16, h2.h)
//                   [14n, 16n)              the same planes of -W
//                   [16n, 16n + 32)         64 bytes whose first word is the fp32 bits of max |w| (s = h2_scale of it; the rest is unspecified)
//                   [16n + 32, 18n + 32)    the two fp16 planes of W 2^s, 32x32x16 order         (X3FragB with two planes; no -W copy)
//
// Inside a region the planes of one fragment interleave: plane p of an element sits 512 p elements behind plane 0 (64 lanes x 8 elements).
#pragma once
#include "h2.h"

enum WplOrder { WPL_32 = 0, WPL_16 = 1 };      // v_mfma_*_32x32x16 / v_mfma_*_16x16x32 fragment order
#define WPL_PLANE 512                          // elements between two planes of one fragment
#define WPL_AMAX_ELEMS 32                      // the 64 bytes kept for the max |w| word

// first element of the copy (order, sign) of the npl-plane form: npl = 1 the bf16 plane, 3 the truncation planes, 2 the fp16 planes
__host__ __device__ constexpr long wpl_region(long n, int npl, WplOrder order, bool neg) {
  return npl == 1 ? 0
       : npl == 3 ? (order == WPL_32 ? (neg ? 3 * n : 0) : (neg ? 9 : 6) * n)
       : order == WPL_16 ? (neg ? 14 : 12) * n : 16 * n + WPL_AMAX_ELEMS;
}
__host__ __device__ constexpr long wpl_amax(long n) { return 16 * n; }      // the max |w| word (mode 4)
// elements of the whole buffer in arithmetic `mode` (lmkd_conv_set_compute_dtype: 1 .. 4)
__host__ __device__ constexpr long wpl_total(long n, int mode) {
  return mode == 1 ? wpl_region(n, 1, WPL_32, false) + n : mode == 4 ? wpl_region(n, 2, WPL_32, false) + 2 * n : wpl_region(n, 3, WPL_16, true) + 3 * n;
}

// the k-slot a lane group of the 16x16x32 order reads (conv_patch16.h: the permutation that frees the LDS patch reads of bank conflicts); self-inverse
__device__ __host__ __forceinline__ constexpr int patch16_kslot(int q) { return ((q & 1) << 1) | (q >> 1); }

// element (col, k) of plane 0 inside a region of npl planes:
//   32x32x16: [col / 32][k / 16][plane][lane = col % 32 + 32 * (k / 8 % 2)][k % 8]
//   16x16x32: [col / 16][k / 32][plane][lane = col % 16 + 16 * kslot(k / 8 % 4)][k % 8]
__host__ __device__ constexpr long wpl_index(WplOrder order, int npl, int Kp, int col, int k) {
  return order == WPL_32 ? ((((long)(col >> 5) * (Kp >> 4) + (k >> 4)) * npl) * 64 + (col & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)
                         : ((((long)(col >> 4) * (Kp >> 5) + (k >> 5)) * npl) * 64 + (col & 15) + 16 * patch16_kslot((k >> 3) & 3)) * 8 + (k & 7);
}

// x = p0 + p1 + p2 exactly, each the TRUNCATION to bf16 of what the ones before left (conv_x3.h); -x has the same planes with the sign bit flipped
__host__ __device__ constexpr void wpl_split3(float x, unsigned short (&p)[3]) {
  const unsigned b0 = __builtin_bit_cast(unsigned, x);
  const float r1 = x - __builtin_bit_cast(float, b0 & 0xffff0000u);
  const unsigned b1 = __builtin_bit_cast(unsigned, r1);
  const float r2 = r1 - __builtin_bit_cast(float, b1 & 0xffff0000u);
  p[0] = (unsigned short)(b0 >> 16);
  p[1] = (unsigned short)(b1 >> 16);
  p[2] = (unsigned short)(__builtin_bit_cast(unsigned, r2) >> 16);
}

// ---- where element (col, k) of the packed weight comes from ----
// an fp32 buffer that is already packed (lmkd_conv2d_pack_weights)
struct WplPacked {
  const float* wp;
  unsigned short* wf;
  int ncols, Kp;
  __device__ __forceinline__ float fetch(int col, int k) const { return wp[(long)col * Kp + k]; }
};
// an OIHW weight and the K-major pack order:
//   mode 0 (forward): col = co, k = (kh * KWp + kw) * Cs + ci   (zero for the padded kw / ci)
//   mode 1 (dgrad)  : col = ci, k = (kh * KW + kw) * Co + co
struct WplOihw {
  const float* w;
  unsigned short* wf;
  int Co, Cin, Cs, KH, KW, KWp, mode, ncols, Kp;
  __host__ __device__ constexpr long index(int col, int k) const {      // into w; -1: padding
    if (mode == 0) {
      const int ci = k % Cs, r = k / Cs;
      const int kw = r % KWp, kh = r / KWp;
      return (ci < Cin && kw < KW) ? (((long)col * Cin + ci) * KH + kh) * KW + kw : -1;
    }
    const int co = k % Co, r = k / Co;
    const int kw = r % KW, kh = r / KW;
    return (((long)co * Cin + col) * KH + kh) * KW + kw;
  }
  __device__ __forceinline__ float fetch(int col, int k) const {
    const long i = index(col, k);
    return i < 0 ? 0.f : w[i];
  }
};

namespace wpl_check {
constexpr long N = 96 * 224;
static_assert(wpl_total(N, 1) == N && wpl_total(N, 2) == 12 * N && wpl_total(N, 3) == 12 * N && wpl_total(N, 4) == 18 * N + 32, "plane buffer totals");
static_assert(wpl_region(N, 3, WPL_32, false) == 0 && wpl_region(N, 3, WPL_32, true) == wpl_region(N, 3, WPL_32, false) + 3 * N &&
              wpl_region(N, 3, WPL_16, false) == wpl_region(N, 3, WPL_32, true) + 3 * N &&
              wpl_region(N, 3, WPL_16, true) == wpl_region(N, 3, WPL_16, false) + 3 * N && wpl_total(N, 2) == wpl_region(N, 3, WPL_16, true) + 3 * N,
              "the four three-plane copies follow one another");
static_assert(wpl_region(N, 2, WPL_16, false) == wpl_total(N, 2) && wpl_region(N, 2, WPL_16, true) == wpl_region(N, 2, WPL_16, false) + 2 * N &&
              wpl_amax(N) == wpl_region(N, 2, WPL_16, true) + 2 * N && wpl_region(N, 2, WPL_32, false) == wpl_amax(N) + WPL_AMAX_ELEMS &&
              wpl_total(N, 4) == wpl_region(N, 2, WPL_32, false) + 2 * N,
              "mode 4 appends the fp16 copies, the maximum and the 32x32x16 fp16 copy");
static_assert(wpl_amax(N) % 2 == 0 && WPL_AMAX_ELEMS % 8 == 0, "the maximum is an aligned word and the last region starts on 16 bytes");
// the last element of a region's last fragment is the region's last element (both orders fill their regions without a gap)
static_assert(wpl_index(WPL_32, 3, 224, 95, 223) + 2 * WPL_PLANE == 3 * N - 1 && wpl_index(WPL_16, 2, 224, 95, 223) + WPL_PLANE == 2 * N - 1, "fragment orders");
constexpr bool split3_exact(float x) {
  unsigned short p[3] = {};
  wpl_split3(x, p);
  return __builtin_bit_cast(float, (unsigned)p[0] << 16) + __builtin_bit_cast(float, (unsigned)p[1] << 16) + __builtin_bit_cast(float, (unsigned)p[2] << 16) == x;
}
static_assert(split3_exact(0.f) && split3_exact(1.f / 3.f) && split3_exact(-0.0499999f) && split3_exact(16777215.f), "the three truncation planes sum to the value");
constexpr WplOihw stem{nullptr, nullptr, 64, 3, 4, 7, 7, 8, 0, 64, 224};
static_assert(stem.index(1, (2 * 8 + 5) * 4 + 2) == ((1 * 3 + 2) * 7 + 2) * 7 + 5 && stem.index(1, 3) == -1 && stem.index(1, 7 * 4) == -1, "pack order, forward");
constexpr WplOihw dgrad{nullptr, nullptr, 64, 32, 32, 3, 3, 3, 1, 32, 576};
static_assert(dgrad.index(5, (1 * 3 + 2) * 64 + 9) == ((9 * 32 + 5) * 3 + 1) * 3 + 2, "pack order, data gradient");
}      // namespace wpl_check

// ---- the writers: every entry of a batch in one launch, blockIdx.y = entry ----
template <class E, int N>
struct WplBatch {
  E e[N];
  int npl;      // 1: the bf16 plane (mode 1); 3: the truncation planes (modes 2 - 4)
  int h2;       // mode 4: the fp16 regions follow
};

// pass 1: the bf16 plane, or the truncation planes of W and -W in both orders; mode 4: also zeroes the max |w| word for pass 2
template <class B>
__global__ void wpl_bf16_kernel(B a) {
  const auto& e = a.e[blockIdx.y];
  const long n = (long)e.ncols * e.Kp;
  if (a.h2 && blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<unsigned*>(e.wf + wpl_amax(n)) = 0u;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int col = (int)(idx / e.Kp), k = (int)(idx - (long)col * e.Kp);
    const float x = e.fetch(col, k);
    if (a.npl == 1) {
      union { __bf16 h; unsigned short u; } c;
      c.h = (__bf16)x;
      e.wf[wpl_index(WPL_32, 1, e.Kp, col, k)] = c.u;
      continue;
    }
    unsigned short p[3];
    wpl_split3(x, p);
#pragma unroll
    for (int order = 0; order < 2; ++order) {
      unsigned short* pos = e.wf + wpl_region(n, 3, (WplOrder)order, false) + wpl_index((WplOrder)order, 3, e.Kp, col, k);
      unsigned short* neg = pos + (wpl_region(n, 3, (WplOrder)order, true) - wpl_region(n, 3, (WplOrder)order, false));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        pos[j * WPL_PLANE] = p[j];
        neg[j * WPL_PLANE] = p[j] ^ 0x8000u;
      }
    }
  }
}
// pass 2 (mode 4): max |w| into its word (the fp32 bits of a non-negative number order like unsigned integers)
template <class B>
__global__ void wpl_amax_kernel(B a) {
  const auto& e = a.e[blockIdx.y];
  const long n = (long)e.ncols * e.Kp;
  float m = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int col = (int)(idx / e.Kp), k = (int)(idx - (long)col * e.Kp);
    m = fmaxf(m, fabsf(e.fetch(col, k)));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned*>(e.wf + wpl_amax(n)), __float_as_uint(m));
}
// pass 3 (mode 4): the fp16 planes of W 2^s (h2.h; s from the word): W and -W in the 16x16x32 order, W in the 32x32x16 order
template <class B>
__global__ void wpl_h2_kernel(B a) {
  const auto& e = a.e[blockIdx.y];
  const long n = (long)e.ncols * e.Kp;
  const float s = h2_scale(*reinterpret_cast<const unsigned*>(e.wf + wpl_amax(n)));
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const int col = (int)(idx / e.Kp), k = (int)(idx - (long)col * e.Kp);
    unsigned short p[2];
    h2_split1(e.fetch(col, k) * s, p[0], p[1]);
    const long o16 = wpl_index(WPL_16, 2, e.Kp, col, k), o32 = wpl_index(WPL_32, 2, e.Kp, col, k);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      e.wf[wpl_region(n, 2, WPL_16, false) + o16 + j * WPL_PLANE] = p[j];
      e.wf[wpl_region(n, 2, WPL_16, true) + o16 + j * WPL_PLANE] = p[j] ^ 0x8000u;
      e.wf[wpl_region(n, 2, WPL_32, false) + o32 + j * WPL_PLANE] = p[j];
    }
  }
}
