// Row LayerNorm, stated once: one workgroup of ROW_THREADS lanes per row, lane t owns the elements t, t + 256, ...  The statistics are
// two-pass (mean, then the centred squares), every sum in a fixed order (lane-strided, block_sum_256): two calls give the same bits, and
// so do the entry points that share this file - mfm.hip (the fusions' LayerNorms), ctx.hip (the CTX keys), trx.hip (the TRX keys and the
// in-place backward of both heads).  The build uses -ffp-contract=off: the expressions below are the arithmetic, as written.
#pragma once
#include "common.h"
#include <type_traits>

#define ROW_THREADS 256

// T* that carries __restrict__ only where R holds
template <bool R, class T> using restrict_if = std::conditional_t<R, T* __restrict__, T*>;

// mean and 1 / sqrt(var + eps) of one row.  first(d) yields element d on the first pass (and may stage it, or store what it gathered on
// the way); at(d) yields it again on the second.  Call with the whole workgroup.
template <class First, class At>
__device__ __forceinline__ void row_stats(First first, At at, int D, float eps, float* red /* 4 floats of LDS */, float& mean, float& rstd) {
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += ROW_THREADS) s += first(d);
  mean = block_sum_256(s, red) / (float)D;
  float q = 0.f;
  for (int d = threadIdx.x; d < D; d += ROW_THREADS) { const float c = at(d) - mean; q += c * c; }
  rstd = 1.f / sqrtf(block_sum_256(q, red) / (float)D + eps);
}

// xhat[d] = (at(d) - mean) * rstd (nullable) ; y[d] = (xhat[d] * gamma[d] + beta[d]) * mask[d] (mask nullable).  y may be the row at() reads:
// a lane reads only the elements it writes, each before it writes it.
template <class At>
__device__ __forceinline__ void row_norm_store(At at, int D, float mean, float rstd, const float* __restrict__ gamma,
                                               const float* __restrict__ beta, const float* __restrict__ mask, float* y, float* __restrict__ xhat) {
  for (int d = threadIdx.x; d < D; d += ROW_THREADS) {
    const float h = (at(d) - mean) * rstd;
    if (xhat) xhat[d] = h;
    const float v = h * gamma[d] + beta[d];
    y[d] = mask ? v * mask[d] : v;
  }
}

// y[r, :] (row stride ldy) = LayerNorm(x[r, :] (+ res[r % res_rows, :])) * gamma + beta (o mask[r, :]).
// KEEP: what the backward reads is stored too, xhat [rows, D] and rstd [rows] (each nullable), and mask (nullable) applies; without it
// the three are not looked at.
// STAGE: the row (with its residual, nullable) is kept in D floats of dynamic LDS between the passes.  Without it the row is read from x
// three times, D is unbounded, there is no residual (res is not read) and y may be x itself: only that instance leaves x and y unqualified.
template <bool STAGE, bool KEEP>
__global__ __launch_bounds__(ROW_THREADS) void ln_fwd_kernel(restrict_if<STAGE, const float> x, const float* __restrict__ res, long res_rows,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mask, restrict_if<STAGE, float> y, long ldy, float* __restrict__ xhat,
                                                             float* __restrict__ rstd_out, int D, float eps) {
  __shared__ float red[4];
  extern __shared__ float row[];
  if constexpr (STAGE && KEEP) __builtin_assume(xhat != nullptr && rstd_out != nullptr);      // lmkd_layernorm_train_fwd requires them
  const long r = blockIdx.x;
  const float* xr = x + r * D;
  const float* rr = STAGE && res ? res + (r % res_rows) * D : nullptr;
  auto first = [&](int d) {
    if constexpr (STAGE) {
      const float v = xr[d] + (rr ? rr[d] : 0.f);
      row[d] = v;
      return v;
    } else {
      return xr[d];
    }
  };
  auto at = [&](int d) { return STAGE ? row[d] : xr[d]; };
  float mean, rstd;
  row_stats(first, at, D, eps, red, mean, rstd);
  row_norm_store(at, D, mean, rstd, gamma, beta, KEEP && mask ? mask + r * D : nullptr, y + r * ldy, KEEP && xhat ? xhat + r * D : nullptr);
  if (KEEP && threadIdx.x == 0 && rstd_out) rstd_out[r] = rstd;
}

// v = dy[r, :] (row stride lddy) o mask[r, :] ; g = v o gamma ; dpre[r, :] = rstd[r] (g - mean(g) - xhat[r, :] mean(g o xhat)) ; dyc[r, :] = v.
// mask and dyc are nullable.
// INPLACE: the gradient is read from dpre itself and overwritten (dy, mask and dyc are not looked at).  That is safe because a lane
// re-reads only the elements it alone writes, each before it writes it.  No two pointers of the kernel alias in either instance: in place
// there is one pointer (dy is null), and out of place lmkd_layernorm_train_bwd rejects dpre == dy and dyc == dy before it launches.
template <bool INPLACE>
__global__ __launch_bounds__(ROW_THREADS) void ln_bwd_kernel(const float* __restrict__ dy, long lddy, const float* __restrict__ mask,
                                                             const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                             const float* __restrict__ gamma, float* __restrict__ dpre, float* __restrict__ dyc,
                                                             int D) {
  __shared__ float red[4];
  const long r = blockIdx.x;
  float* out = dpre + r * D;
  const float* gr = INPLACE ? out : dy + r * lddy;
  const float* mr = !INPLACE && mask ? mask + r * D : nullptr;
  const float* h = xhat + r * D;
  float s1 = 0.f, s2 = 0.f;
  for (int d = threadIdx.x; d < D; d += ROW_THREADS) {
    const float v = mr ? gr[d] * mr[d] : gr[d];
    if (!INPLACE && dyc) dyc[r * D + d] = v;
    const float g = v * gamma[d];
    s1 += g;
    s2 += g * h[d];
  }
  const float m1 = block_sum_256(s1, red) / (float)D;
  const float m2 = block_sum_256(s2, red) / (float)D;
  const float rs = rstd[r];
  for (int d = threadIdx.x; d < D; d += ROW_THREADS) {
    const float v = mr ? gr[d] * mr[d] : gr[d];
    out[d] = rs * (v * gamma[d] - m1 - h[d] * m2);
  }
}
