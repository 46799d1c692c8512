// Implicit-GEMM 2-D convolution on the fp32 MFMA tile engine, NHWC activations.
//
//   forward      y[n,oh,ow,co]   = sum_{kh,kw,ci} x[n,oh*s+kh-p,ow*s+kw-p,ci] * W[co,ci,kh,kw]
//   data grad    dx[n,ih,iw,ci]  = sum_{kh,kw,co} dy[n,(ih+p-kh)/s,(iw+p-kw)/s,co] * W[co,ci,kh,kw]
//   weight grad  dW[co,ci,kh,kw] = sum_{n,oh,ow}  dy[n,oh,ow,co] * x[n,oh*s+kh-p,ow*s+kw-p,ci]
//
// forward and data-grad share one kernel: GEMM rows = output pixels, GEMM cols = output
// channels, K = (tap, channel) of the gathered tensor; a per-class tap table {dh,dw,kofs}
// describes which source pixel / packed-weight slice each K-step reads.  Stride-2 data-grad
// enumerates its rows per input-parity class (4 classes), so every tile only runs the taps
// that are non-zero for its parity (no wasted MFMAs on the zero-stuffed positions).
// The 7x7 stem (Cin=3) runs on a channel-padded NHWC4 input: one K-step = one kernel row
// (8 taps x 4 channels = 32 contiguous floats of the input).
// Train-mode BatchNorm statistics (sum, sum of squares per channel) are reduced from the
// accumulators in the forward epilogue into per-row-tile partials (deterministic).
#include "gemm_core.h"
#include <atomic>
#include <mutex>

struct ConvGemmArgs {
  const float* src;
  const float* wpk;
  float* out;
  float* stat_partial;
  int N, Hs, Ws, Cs;
  int Hr, Wr, rows_per_class, tiles_per_class;
  int sh;
  int Ho, Wo, Co, omul;
  int Kp, cps, nclass;
  int n_rt, n_ct, xcd_mode;   // row tiles (all classes), column tiles, tile order (XCD-aware 1-D grid, see xcd_decode)
  int taps_pm1;               // conv_patch.h: every tap of every class lies within +-1 pixel (3x3 / 1x1 launches): the per-row tap masks come from a table
  int grid_step;              // persistent launches: gridDim.x (read from the argument block's LDS copy; gridDim itself is another scalar load from the segment)
  int grid_total;             // persistent launches (conv_patch.h): slots of the tile order, xcd_grid(n_rt, n_ct, xcd_mode); a workgroup walks slots blockIdx.x + k gridDim.x
  int same;    // (not read: the host plans same-size convolutions, plan_fwd / plan_dgrad; kept so the argument layout stays put)
  int halo;    // conv_patch_x3_kernel: largest |dh * Ws + dw| over the taps (pixels either side of the tile's own range)
  int accum;   // epilogue: out = acc + out (residual-branch gradient already sits in the output buffer)
  // STATS == 2 (inference): out = relu?( acc * scale[c] + shift[c] (+ res) ), scale/shift = rows 2/3 of the [5][C] BatchNorm table
  const float* ep_stats;
  const float* ep_res;
  int ep_relu;
  // PRE (training): src holds the RAW output of the previous convolution; the loader applies that layer's train-mode BatchNorm
  // and ReLU, relu(fmaf(v, scale[c], shift[c])) with scale/shift = rows 2/3 of its [5][C] table, while it fills LDS - the
  // normalised activation never exists in HBM.  Zero padding stays zero (it pads the activation, not the raw tensor).
  const float* pre_stats;
  // data gradient whose result feeds relu + train-mode BatchNorm backward (lmkd_conv2d_bwd_data_bn): bnb_x = that BatchNorm's input (the
  // raw convolution output, shaped like `out`), bnb_stats = its [5][Co] table; stat_partial then receives per row tile
  // (sum g, sum g * xhat), g = out * [fma(x, scale, shift) > 0], xhat = (x - mean) * invstd - what bn_bwd_reduce_kernel sums
  const float* bnb_x;
  const float* bnb_stats;
  // SRC2 (conv_patch16.h): stride-2 forward convolution as four same-size convolutions over the input's parity classes.  Hs / Ws then
  // hold the CLASS grid (= the output grid), s2_wfull the input's width, s2_off[c] the element offset of class c's origin
  // ((sph * W + spw) * Cs) and taps[0][s2_t0[c] .. s2_t0[c + 1] - 1] the taps of class c (dh / dw in the class grid)
  int src2, s2_ncls, s2_wfull;
  int s2_t0[5], s2_off[4];
  // Two frame segments in one launch (round 4: the support-frame and the query-frame trunk call of an episode, resnet18_2fc.py:41-42, as
  // ONE tensor [F0 + F1, H, W, C]): rows [0, seg_m0) of a class belong to segment 0, the rest to segment 1.  The row tiles are dealt per
  // segment - tiles [0, seg_t0) cover segment 0, tile seg_t0 starts at row seg_m0 - so no tile straddles the boundary: every tile's
  // BatchNorm partial sums belong to one segment, the [2][5][C] tables (pre_stats, bnb_stats) are indexed by the tile's segment, and the
  // tiles (with their -W halves, x3_neg_tile) are exactly those of two separate launches: bit-identical results.
  // Unsegmented launch: seg_m0 = rows_per_class, seg_t0 = tiles_per_class (conv_set_tiles).
  int seg_m0, seg_t0;
  const unsigned* h2_xw;      // two-plane fp16 arithmetic (compute dtype 4): the word holding max |operand| (lmkd_conv_operand_amax); null: three bf16 planes
  unsigned* amax_out;         // conv_patch16_x3_kernel: fold max |out| into these words (lmkd_conv_output_amax); null: not recorded
  FastDiv div_hw, div_w;
  int ntap[LMKD_MAX_CLASSES];
  Tap taps[LMKD_MAX_CLASSES][LMKD_MAX_TAPS];
};

// tile -> first row, row limit, segment, index / count of the tile inside its segment (ConvGemmArgs::seg_m0)
struct SegTile { int row0, mend, seg, ltile, ltiles; };
__device__ __forceinline__ SegTile seg_tile(const ConvGemmArgs& a, int tile, int BM) {
  SegTile s;
  if (tile < a.seg_t0) { s.row0 = tile * BM; s.mend = a.seg_m0; s.seg = 0; s.ltile = tile; s.ltiles = a.seg_t0; }
  else { s.row0 = a.seg_m0 + (tile - a.seg_t0) * BM; s.mend = a.rows_per_class; s.seg = 1; s.ltile = tile - a.seg_t0; s.ltiles = a.tiles_per_class - a.seg_t0; }
  return s;
}
// host: row tiles of a launch with BM rows per tile (per class), segment-aware
static inline void conv_set_tiles(ConvGemmArgs& a, int BM) {
  if (a.seg_m0 <= 0 || a.seg_m0 >= a.rows_per_class) a.seg_m0 = a.rows_per_class;
  a.seg_t0 = (a.seg_m0 + BM - 1) / BM;
  a.tiles_per_class = a.seg_t0 + (a.rows_per_class - a.seg_m0 + BM - 1) / BM;
  a.n_rt = a.nclass * a.tiles_per_class;
}

// K-major implicit-im2col loader (rows = output pixels of this tile).
template <int ROWS, bool SMALLC, int THREADS = LMKD_THREADS, bool PRE = false>
struct LoaderConvGather {
  static constexpr bool ROWK = true;
  static constexpr int RPP = THREADS / 8;
  static constexpr int NI = ROWS / RPP;
  static constexpr int LD = LMKD_LDK;
  static constexpr int LDS_FLOATS = ROWS * LMKD_LDK;
  int base[NI], hw[NI];
  float4 reg[NI];
  const float* src;
  int Hs, Ws, Cs, kc4;
  float4 psc, psh;      // PRE: BatchNorm scale / shift of this lane's 4 channels of the current 32-channel chunk
  unsigned inb;         // PRE: which of the NI prefetched rows are real pixels (zero padding must stay zero)
  // the chunk's table entries: fetched once per chunk (the K loop runs the taps of one chunk back to back).  Like the tile
  // loads they are only CONSUMED in store(), after the MFMAs of the current K-step: nothing waits for memory in between.
  __device__ __forceinline__ void load_pre(const float* __restrict__ stats, int coff) {
    psc = *reinterpret_cast<const float4*>(stats + 2 * Cs + coff + kc4);
    psh = *reinterpret_cast<const float4*>(stats + 3 * Cs + coff + kc4);
  }
  __device__ __forceinline__ void init(const float* src_, int Hs_, int Ws_, int Cs_, const int* s_src, const int* s_hw) {
    const int tid = threadIdx.x;
    src = src_; Hs = Hs_; Ws = Ws_; Cs = Cs_;
    kc4 = (tid & 7) * 4;
    inb = 0u;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      base[i] = s_src[(tid >> 3) + RPP * i];
      hw[i] = s_hw[(tid >> 3) + RPP * i];
    }
  }
  // tap: this step's {dh,dw}; coff: channel offset inside the tap (multiple of 32)
  __device__ __forceinline__ void load(int dh, int dw, int coff) {
    const int dwe = SMALLC ? dw + (kc4 >> 2) : dw;
    const int rel = (dh * Ws + dwe) * Cs + (SMALLC ? 0 : coff + kc4);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int h = (hw[i] >> 16) + dh, w = (hw[i] & 0xffff) + dwe;
      if (hw[i] >= 0 && (unsigned)h < (unsigned)Hs && (unsigned)w < (unsigned)Ws) {
        reg[i] = *reinterpret_cast<const float4*>(src + (long)(base[i] + rel));
        if (PRE) inb |= 1u << i;
      } else {
        reg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (PRE) inb &= ~(1u << i);
      }
    }
  }
  __device__ __forceinline__ void store(float* S) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float4 v = reg[i];
      if (PRE && ((inb >> i) & 1u)) {      // the same operations as bn_apply_kernel: bit-identical to the materialised activation
        v.x = fmaxf(fmaf(v.x, psc.x, psh.x), 0.f); v.y = fmaxf(fmaf(v.y, psc.y, psh.y), 0.f);
        v.z = fmaxf(fmaf(v.z, psc.z, psh.z), 0.f); v.w = fmaxf(fmaf(v.w, psc.w, psh.w), 0.f);
      }
      *reinterpret_cast<float4*>(S + ((tid >> 3) + RPP * i) * LMKD_LDK + kc4) = v;
    }
  }
};

// Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2) in linear id order.  The tile order is
// chosen so that what one XCD touches at a time fits its L2 (PMC: the naive order re-fetched every input row ~6x):
//   mode 0 (row bands): XCD x owns a contiguous band of row tiles and walks it in order, column tiles fastest.  The 3x3
//          halo rows shared by neighbouring row tiles and the A tile shared by the column tiles are then L2 hits.
//   mode 1 (column slices, n_ct a multiple of 8): XCD x owns column tiles x, x+8, ...: it keeps re-reading ONE slice of
//          the packed weights (layer 4: 9.4 MB of weights, 1.2 MB per 64-column slice) while streaming the small A.
// Pure speed hint: any placement computes the same tiles.
static int g_xcd_mode = -1;   // -1 auto
extern "C" int lmkd_conv_set_xcd_mode(int m) { g_xcd_mode = m; return LMKD_OK; }

__device__ __forceinline__ bool xcd_decode(int L, int n_rt, int n_ct, int mode, int& rt, int& ct) {
  const int x = L & 7, j = L >> 3;
  if (mode == 1) {
    ct = x + 8 * (j / n_rt);
    rt = j - (j / n_rt) * n_rt;
    return ct < n_ct;
  }
  const int chunk = (n_rt + 7) >> 3;
  ct = j % n_ct;
  const int rl = j / n_ct;
  rt = x * chunk + rl;
  return rl < chunk && rt < n_rt;
}
static inline int xcd_grid(int n_rt, int n_ct, int mode) {
  if (mode == 1) return n_rt * n_ct;
  return 8 * cdiv(n_rt, 8) * n_ct;
}

template <class Cfg, bool SMALLC, int STATS, bool BF16, bool PRE = false>   // STATS: 0 plain store, 1 + BatchNorm partial sums, 2 BatchNorm-affine (+residual, ReLU) epilogue
__global__ __launch_bounds__(Cfg::THREADS) void conv_gemm_kernel(ConvGemmArgs a) {
  using LA = LoaderConvGather<Cfg::BM, SMALLC, Cfg::THREADS, PRE>;
  using LB = LoaderKMajorDense<Cfg::BN, Cfg::THREADS>;   // packed weights are K-major: Wp[col][k]
  __shared__ __attribute__((aligned(16))) float smem[2 * (LA::LDS_FLOATS + LB::LDS_FLOATS)];
  __shared__ int s_src[Cfg::BM], s_hw[Cfg::BM], s_out[Cfg::BM];
  __shared__ float s_red[STATS == 1 ? Cfg::WM * Cfg::BN * 2 : 1];

  const int tid = threadIdx.x;
  int rt, ct;
  if (!xcd_decode(blockIdx.x, a.n_rt, a.n_ct, a.xcd_mode, rt, ct)) return;
  // parity classes interleaved (stride-2 data gradient: the classes run 1, 2, 2 and 4 taps): every XCD band and every
  // stretch of the dispatch order then carries the same mix of light and heavy tiles
  const int tile = rt / a.nclass;
  const int cls = rt - tile * a.nclass;
  const int ph = cls >> 1, pw = cls & 1;
  if (a.accum && a.ntap[cls] == 0) return;      // out += 0: a parity class no tap reaches (1x1 stride-2 data gradient)
  const int row0 = tile * Cfg::BM, n0 = ct * Cfg::BN;
  for (int r = tid; r < Cfg::BM; r += Cfg::THREADS) {
    const int m = row0 + r;
    bool ok = m < a.rows_per_class;
    int n = 0, aa = 0, bb = 0;
    if (ok) {
      n = fdiv(m, a.div_hw);
      const int rem = m - n * a.Hr * a.Wr;
      aa = fdiv(rem, a.div_w);
      bb = rem - aa * a.Wr;
      // odd H or W in the stride-2 data gradient: the odd-parity classes have one row/column fewer
      ok = (aa * a.omul + ph) < a.Ho && (bb * a.omul + pw) < a.Wo;
    }
    if (ok) {
      s_src[r] = ((n * a.Hs + aa * a.sh) * a.Ws + bb * a.sh) * a.Cs;
      s_hw[r] = ((aa * a.sh) << 16) | (bb * a.sh);
      s_out[r] = ((n * a.Ho + aa * a.omul + ph) * a.Wo + bb * a.omul + pw) * a.Co;
    } else {
      s_src[r] = 0;
      s_hw[r] = -1;
      s_out[r] = -1;
    }
  }
  __syncthreads();
  LA la;
  LB lb;
  la.init(a.src, a.Hs, a.Ws, a.Cs, s_src, s_hw);
  lb.init(a.wpk, a.Kp, n0, a.Co, a.Kp);

  f32x16 acc[Cfg::TM][Cfg::TN];
  const int nk = a.ntap[cls] * a.cps;
  {
    // hand-inlined gemm_mainloop: the two loaders take different per-step arguments
    constexpr int SA = LA::LDS_FLOATS, SB = LB::LDS_FLOATS;
    float* As0 = smem;
    float* Bs0 = smem + 2 * SA;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / Cfg::WN, wn = wave % Cfg::WN;
    const int h = lane >> 5;
    const int a_row = wm * (Cfg::TM * 32) + (lane & 31);
    const int b_row = wn * (Cfg::TN * 32) + (lane & 31);
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const Tap* taps = a.taps[cls];
    const int ntap_c = a.ntap[cls];
    auto issue = [&](int t) {
      // K order: channel chunk outer, tap inner.  The taps of one 32-channel chunk read the same 128-byte pixel segments (shifted
      // by a pixel), so the 9x reuse of a 3x3 conv sits in consecutive K-steps and stays in L1/L2; tap-major order re-fetched
      // the wide rows of layer 4 (2 KB per pixel) once per tap: PMC FETCH_SIZE 790-1080 MB per launch for 50 MB of operands.
      const int cc = t / ntap_c, tp = t - cc * ntap_c;
      const Tap tap = taps[tp];
      if (PRE && tp == 0) la.load_pre(a.pre_stats, cc * LMKD_BK);
      la.load(tap.dh, tap.dw, cc * LMKD_BK);
      lb.load(tap.kofs + cc * LMKD_BK);
    };
    if (nk > 0) {
      issue(0);
      la.store(As0);
      lb.store(Bs0);
      __syncthreads();
      // last K-step peeled: no condition sits between a tile's prefetch and its LDS store inside the loop (with one, hipcc
      // copies the prefetched registers in front of the MFMAs - and waits for the loads there - in the PRE instances)
      for (int t = 0; t + 1 < nk; ++t) {
        const int cur = t & 1;
        issue(t + 1);
        if (BF16) mfma_kstep_bf16<Cfg, LA, LB>(As0 + cur * SA, Bs0 + cur * SB, a_row, b_row, h, acc);
        else mfma_kstep<Cfg, LA, LB>(As0 + cur * SA, Bs0 + cur * SB, a_row, b_row, h, acc);
        // keep the store side (incl. the PRE loader's BatchNorm+ReLU arithmetic) BEHIND the MFMAs: hoisted above them it drags the
        // s_waitcnt vmcnt(0) of the prefetched tile in front of the matrix work and the prefetch hides nothing
        __builtin_amdgcn_sched_barrier(0);
        la.store(As0 + (cur ^ 1) * SA);
        lb.store(Bs0 + (cur ^ 1) * SB);
        __syncthreads();
      }
      const int last = (nk - 1) & 1;
      if (BF16) mfma_kstep_bf16<Cfg, LA, LB>(As0 + last * SA, Bs0 + last * SB, a_row, b_row, h, acc);
      else mfma_kstep<Cfg, LA, LB>(As0 + last * SA, Bs0 + last * SB, a_row, b_row, h, acc);
    }
  }

  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / Cfg::WN, wn = wave % Cfg::WN;
  const int cl0 = wn * (Cfg::TN * 32) + (lane & 31);
  if (STATS == 0 && a.accum) {
    // out += acc: fetch the whole tile's previous values first (independent loads in flight together), then add; the
    // per-element "load, wait, add, store" form serialised 16 dependent global round trips per wave
    float prev[Cfg::TM][Cfg::TN][16];
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ob = s_out[wm * (Cfg::TM * 32) + i * 32 + acc_row(e, lane)];
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
          const int col = n0 + cl0 + j * 32;
          prev[i][j][e] = (ob >= 0 && col < a.Co) ? a.out[(long)ob + col] : 0.f;
        }
      }
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = acc[i][j][e] + prev[i][j][e];
  }
  float s1[Cfg::TN], s2[Cfg::TN];
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j) s1[j] = s2[j] = 0.f;
  float esc[Cfg::TN], esh[Cfg::TN];
  if (STATS == 2) {
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const int col = n0 + cl0 + j * 32;
      esc[j] = col < a.Co ? a.ep_stats[2 * a.Co + col] : 0.f;
      esh[j] = col < a.Co ? a.ep_stats[3 * a.Co + col] : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int rl = wm * (Cfg::TM * 32) + i * 32 + acc_row(e, lane);
      const int ob = s_out[rl];
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j) {
        const int col = n0 + cl0 + j * 32;
        float v = acc[i][j][e];
        if (ob >= 0 && col < a.Co) {
          float* o = a.out + (long)ob + col;
          if (STATS == 2) {   // same operations, in the same order, as bn_apply_kernel: bit-identical to the two-pass form
            v = fmaf(v, esc[j], esh[j]);
            if (a.ep_res) v += a.ep_res[(long)ob + col];
            if (a.ep_relu) v = fmaxf(v, 0.f);
            *o = v;
          } else {
            *o = (STATS == 1 && a.accum) ? v + *o : v;      // STATS == 0: the previous values were added above
          }
        }
        if (STATS == 1) { s1[j] += v; s2[j] = fmaf(v, v, s2[j]); }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (STATS == 1) {
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const float t1 = s1[j] + __shfl_xor(s1[j], 32, 64);
      const float t2 = s2[j] + __shfl_xor(s2[j], 32, 64);
      if (lane < 32) {
        s_red[(wm * Cfg::BN + cl0 + j * 32) * 2 + 0] = t1;
        s_red[(wm * Cfg::BN + cl0 + j * 32) * 2 + 1] = t2;
      }
    }
  }
  if (STATS == 1) {
    __syncthreads();
    if (tid < Cfg::BN && n0 + tid < a.Co) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < Cfg::WM; ++w) {
        s1 += s_red[(w * Cfg::BN + tid) * 2 + 0];
        s2 += s_red[(w * Cfg::BN + tid) * 2 + 1];
      }
      float* p = a.stat_partial + ((long)rt * a.Co + n0 + tid) * 2;
      p[0] = s1;
      p[1] = s2;
    }
  }
}

#include "wplanes.h"
#include "conv_x3.h"
#include "conv_patch.h"
#include "conv_patch16.h"
#include "conv_stem.h"

// ---------------------------------------------------------------------------------
// weight gradient: rows = co (dy, K-outer), cols = packed (tap, ci), K = pixels, split-K slabs
// ---------------------------------------------------------------------------------
struct WgradArgs {
  const float* dy;
  const float* x;
  float* slab;
  int N, Hs, Ws, Cs, Ho, Wo, Co;
  int stride, pad, KH, KW, KWp;
  int Kp, Mpix, steps_total, steps_per_split;
  int n_mt, n_jt, splits, xcd_mode;   // 1-D grid decode (xcd_mode 1: all tiles of pixel split z run on XCD z % 8)
  const float* pre_stats;             // PRE: x is a raw conv output; the loader applies relu(BatchNorm(x)) (see ConvGemmArgs)
  int seg_pix0, seg_splits0, sps1;    // two frame segments (wgrad_win.h WgradWinArgs): conv_wgrad_x3_kernel only; one segment: Mpix, splits, 0
  FastDiv div_hw, div_w;
  const unsigned* h2_xw;              // two-plane fp16 form (conv_wgrad_x3_kernel<.., 3, ..>): the maxima of x / dy (lmkd_conv_operand_amax)
  const unsigned* h2_dyw;
};

// split z -> first pixel, pixel limit, number of 32-pixel steps, segment
struct WinSlab { int kfirst, kend, nk, seg; };
__device__ __forceinline__ WinSlab win_slab(int z, int Mpix, int sps0, int seg_pix0, int seg_splits0, int sps1) {
  WinSlab w;
  int sps;
  if (z < seg_splits0) { w.kfirst = z * sps0 * LMKD_BK; w.kend = seg_pix0; w.seg = 0; sps = sps0; }
  else { w.kfirst = seg_pix0 + (z - seg_splits0) * sps1 * LMKD_BK; w.kend = Mpix; w.seg = 1; sps = sps1; }
  const int left = (w.kend - w.kfirst + LMKD_BK - 1) / LMKD_BK;
  w.nk = left < sps ? (left < 0 ? 0 : left) : sps;
  return w;
}

template <int ROWS, bool SMALLC, int THREADS = LMKD_THREADS, bool PRE = false>
struct LoaderWgradGather {
  static constexpr bool ROWK = false;
  static constexpr int LD = ROWS;
  static constexpr int LDS_FLOATS = LMKD_BK * LD;
  static constexpr int CPR = ROWS / 4;
  static constexpr int KPP = THREADS / CPR;
  static constexpr int NI = LMKD_BK / KPP;
  const float* x;
  FastDiv div_hw, div_w;
  int Mpix, HoWo, Wo, Hs, Ws, Cs, stride;
  float4 reg[NI];
  int dh, dw, coff, r4;
  bool tap_ok;
  float4 psc, psh;
  unsigned inb;      // PRE: rows of the prefetched slab that are real pixels; the transform runs in store(), behind the MFMAs
  __device__ __forceinline__ void init(const WgradArgs& a, int j0) {
    inb = 0u;
    x = a.x; div_hw = a.div_hw; div_w = a.div_w;
    Mpix = a.Mpix; HoWo = a.Ho * a.Wo; Wo = a.Wo; Hs = a.Hs; Ws = a.Ws; Cs = a.Cs; stride = a.stride;
    const int tid = threadIdx.x;
    r4 = (tid % CPR) * 4;
    const int col = j0 + r4;
    if (SMALLC) {  // col -> (kh = col/32, kw = (col%32)/4), 4 channels per tap
      const int kh = col >> 5, kw = (col & 31) >> 2;
      dh = kh - a.pad; dw = kw - a.pad; coff = 0;
      tap_ok = kh < a.KH && kw < a.KW && col < a.Kp;
    } else {
      const int tap = col / a.Cs;
      coff = col - tap * a.Cs;
      const int kh = tap / a.KWp, kw = tap - kh * a.KWp;
      dh = kh - a.pad; dw = kw - a.pad;
      tap_ok = col < a.Kp && kw < a.KW;
    }
    if (PRE && tap_ok) {      // this thread's 4 channels never change over the pixel loop
      psc = *reinterpret_cast<const float4*>(a.pre_stats + 2 * a.Cs + coff);
      psh = *reinterpret_cast<const float4*>(a.pre_stats + 3 * a.Cs + coff);
    }
  }
  __device__ __forceinline__ void load(int koff) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int p = koff + tid / CPR + KPP * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (tap_ok && p < Mpix) {
        const int n = fdiv(p, div_hw);
        const int rem = p - n * HoWo;
        const int oh = fdiv(rem, div_w);
        const int ow = rem - oh * Wo;
        const int h = oh * stride + dh, w = ow * stride + dw;
        if ((unsigned)h < (unsigned)Hs && (unsigned)w < (unsigned)Ws) {
          v = *reinterpret_cast<const float4*>(x + ((long)(n * Hs + h) * Ws + w) * Cs + coff);
          if (PRE) inb |= 1u << i;
        } else if (PRE) inb &= ~(1u << i);
      } else if (PRE) inb &= ~(1u << i);
      reg[i] = v;
    }
  }
  __device__ __forceinline__ void store(float* S) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      int k = tid / CPR + KPP * i;
      float4 v = reg[i];
      if (PRE && ((inb >> i) & 1u)) {
        v.x = fmaxf(fmaf(v.x, psc.x, psh.x), 0.f); v.y = fmaxf(fmaf(v.y, psc.y, psh.y), 0.f);
        v.z = fmaxf(fmaf(v.z, psc.z, psh.z), 0.f); v.w = fmaxf(fmaf(v.w, psc.w, psh.w), 0.f);
      }
      *reinterpret_cast<float4*>(S + k * LD + r4) = v;
    }
  }
};

template <class Cfg, bool SMALLC, bool BF16, bool PRE = false>
__global__ __launch_bounds__(Cfg::THREADS) void conv_wgrad_kernel(WgradArgs a) {
  using LA = LoaderMMajorDense<Cfg::BM, Cfg::THREADS>;
  using LB = LoaderWgradGather<Cfg::BN, SMALLC, Cfg::THREADS, PRE>;
  __shared__ __attribute__((aligned(16))) float smem[2 * (LA::LDS_FLOATS + LB::LDS_FLOATS)];
  // Tile order.  The 9 column tiles (taps) of one pixel split read the same x rows and the same dy rows; in plain order
  // they land on different XCDs and every XCD fetches those rows again (PMC: 2.6-3.1 GB per launch on the 160 MB layers).
  // With many splits, all tiles of split z are given ids congruent mod 8 so that one XCD's L2 serves them.
  int z, tz;
  const int tiles_per_z = a.n_mt * a.n_jt;
  if (a.xcd_mode) {
    const int xj = blockIdx.x >> 3;
    z = (blockIdx.x & 7) + 8 * (xj / tiles_per_z);
    if (z >= a.splits) return;
    tz = xj - (xj / tiles_per_z) * tiles_per_z;
  } else {
    z = blockIdx.x / tiles_per_z;
    tz = blockIdx.x - z * tiles_per_z;
  }
  const int m0 = (tz % a.n_mt) * Cfg::BM, j0 = (tz / a.n_mt) * Cfg::BN;
  LA la;
  LB lb;
  la.init(a.dy, a.Co, m0, a.Co, a.Mpix);
  lb.init(a, j0);
  const int s0 = z * a.steps_per_split;
  int nk = a.steps_total - s0;
  if (nk > a.steps_per_split) nk = a.steps_per_split;
  f32x16 acc[Cfg::TM][Cfg::TN];
  auto koff = [s0](int t) { return (s0 + t) * LMKD_BK; };
  gemm_mainloop<Cfg, LA, LB, decltype(koff), decltype(koff), BF16, PRE>(la, lb, nk, koff, koff, smem, acc);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / Cfg::WN, wn = wave % Cfg::WN;
  float* C = a.slab + (long)z * a.Co * a.Kp;
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j) {
    const int col = j0 + wn * (Cfg::TN * 32) + j * 32 + (lane & 31);
    if (col >= a.Kp) continue;
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * (Cfg::TM * 32) + i * 32 + acc_row(e, lane);
        if (row < a.Co) C[(long)row * a.Kp + col] = acc[i][j][e];
      }
  }
}

// dW (OIHW) = sum over split slabs of slab[z][co][(kh*KWp+kw)*Cs + ci]  (coalesced slab reads, 8 loads in flight per
// thread; the scattered 4-byte OIHW writes are ~11 M floats per trunk call in total)
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw, int splits, int Co, int Cin,
                                    int Cs, int KH, int KW, int KWp, int Kp, int accumulate) {
  const long total = (long)Co * KH * KW * Cin;
  const long zs = (long)Co * Kp;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int ci = idx % Cin;
    long r = idx / Cin;
    const int kw = r % KW; r /= KW;
    const int kh = r % KH;
    const int co = r / KH;
    const float* p = slab + (long)co * Kp + (long)(kh * KWp + kw) * Cs + ci;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int z = 0;
    for (; z + 8 <= splits; z += 8) {
      const float a0 = p[(z + 0) * zs], a1 = p[(z + 1) * zs], a2 = p[(z + 2) * zs], a3 = p[(z + 3) * zs];
      const float a4 = p[(z + 4) * zs], a5 = p[(z + 5) * zs], a6 = p[(z + 6) * zs], a7 = p[(z + 7) * zs];
      s0 += a0; s1 += a1; s2 += a2; s3 += a3; s0 += a4; s1 += a5; s2 += a6; s3 += a7;
    }
    for (; z < splits; ++z) s0 += p[z * zs];
    float* o = dw + (((long)co * Cin + ci) * KH + kh) * KW + kw;
    const float v = (s0 + s1) + (s2 + s3);
    *o = accumulate ? *o + v : v;      // accumulate: dw is weight.grad itself (gradient accumulation over trunk calls / episodes)
  }
}

// The same reduction for the stem (round 5; Kp = 7 x 8 x 4 = 224 <= 256, several hundred slabs - one per workgroup of stem_wgrad_kernel): one workgroup per
// output channel, thread (k, q) adds the slabs q, q + 4, ... of K position k (coalesced rows of Kp floats), the four partial sums meet in
// LDS.  wgrad_reduce_kernel gave the 9 408 weights one thread each for a walk over every slab: 184 us.
__global__ __launch_bounds__(1024) void wgrad_reduce_stem_kernel(const float* __restrict__ slab, float* __restrict__ dw, int splits, int Co, int Cin,
                                                                 int Cs, int KH, int KW, int KWp, int Kp, int accumulate) {
  __shared__ float sm[4][256];
  const int k = threadIdx.x, q = threadIdx.y, co = blockIdx.x;
  const long zs = (long)Co * Kp;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (k < Kp) {
    const float* p = slab + (long)co * Kp + k;
    int z = q;
    for (; z + 28 < splits; z += 32) {
      const float a0 = p[(z + 0) * zs], a1 = p[(z + 4) * zs], a2 = p[(z + 8) * zs], a3 = p[(z + 12) * zs];
      const float a4 = p[(z + 16) * zs], a5 = p[(z + 20) * zs], a6 = p[(z + 24) * zs], a7 = p[(z + 28) * zs];
      s0 += a0; s1 += a1; s2 += a2; s3 += a3; s0 += a4; s1 += a5; s2 += a6; s3 += a7;
    }
    for (; z < splits; z += 4) s0 += p[z * zs];
  }
  sm[q][k] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (q == 0 && k < Kp) {
    const int ci = k % Cs, r = k / Cs;
    const int kw = r % KWp, kh = r / KWp;
    if (ci < Cin && kw < KW && kh < KH) {
      const float v = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
      float* o = dw + (((long)co * Cin + ci) * KH + kh) * KW + kw;
      *o = accumulate ? *o + v : v;
    }
  }
}
// (a form that transposed 64 x 9 results through LDS into contiguous OIHW runs, one workgroup per output channel and 64 input channels,
// measured 48 % SLOWER than this kernel's scattered 4-byte stores - 9.87 vs 6.66 ms over the 247 non-stem launches of 13 episodes,
// profiles/r05_kernel_stats_serial_f32.csv of that build: the time is the slabs' read, and a third of its lanes idled in the last pass)
static void launch_wgrad_reduce(const float* slab, float* dw, int splits, int Co, int Cin, int Cs, int KH, int KW, int KWp, int Kp,
                                int accumulate, hipStream_t s) {
  const long total = (long)Co * KH * KW * Cin;
  int rg = cdiv(total, 256);
  if (rg > 4096) rg = 4096;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(rg), dim3(256), 0, s, slab, dw, splits, Co, Cin, Cs, KH, KW, KWp, Kp, accumulate);
}

#include "wgrad_x3.h"
#include "wgrad_win.h"
#include "wgrad_stem.h"

// K-major packed weights (the GEMM's B operand: one row of K per output column) in the pack order of wplanes.h (WplOihw)
__global__ void pack_weights_kernel(WplOihw e, float* __restrict__ wp) {
  const long total = (long)e.ncols * e.Kp;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int col = (int)(idx / e.Kp);
    wp[idx] = e.fetch(col, (int)(idx - (long)col * e.Kp));
  }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
static inline int conv_out(int H, int K, int s, int p) { return (H + 2 * p - K) / s + 1; }
static inline int kw_padded(int Cs, int KW) { return Cs >= 32 ? KW : ((KW * Cs + 31) / 32) * 32 / Cs; }

// the source of a weight's packed elements: dims as the entry points take them; ncols x Kp is the packed weight
static WplOihw wpl_oihw(const float* w, void* wf, int Cout, int Cin, int Cs, int KH, int KW, int mode) {
  const int KWp = kw_padded(Cs, KW);
  return WplOihw{w, (unsigned short*)wf, Cout, Cin, Cs, KH, KW, KWp, mode, mode == 0 ? Cout : Cin, mode == 0 ? KH * KWp * Cs : KH * KW * Cout};
}

extern "C" long lmkd_conv2d_packed_weight_elems(int Cout, int Cin, int Cs, int KH, int KW, int mode) {
  const WplOihw e = wpl_oihw(nullptr, nullptr, Cout, Cin, Cs, KH, KW, mode);
  return (long)e.ncols * e.Kp;
}

extern "C" int lmkd_conv2d_pack_weights(const float* w_oihw, float* wp, int Cout, int Cin, int Cs, int KH, int KW,
                                        int mode, void* stream) {
  LMKD_REQUIRE(w_oihw && wp, "lmkd_conv2d_pack_weights: null pointer");
  LMKD_REQUIRE(mode == 0 || mode == 1, "lmkd_conv2d_pack_weights: mode must be 0 (fwd) or 1 (dgrad)");
  LMKD_REQUIRE(Cs >= Cin && (Cs % 32 == 0 || Cs == 4), "lmkd_conv2d_pack_weights: Cs=%d must be 4 or a multiple of 32", Cs);
  const WplOihw e = wpl_oihw(w_oihw, nullptr, Cout, Cin, Cs, KH, KW, mode);
  int grid = cdiv((long)e.ncols * e.Kp, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(pack_weights_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, e, wp);
  LMKD_CHECK_LAUNCH("lmkd_conv2d_pack_weights");
  return LMKD_OK;
}

// ---- compute dtype of the convolutions (lmkd_conv_set_compute_dtype): 0 = exact fp32 MFMA, 1 = bf16 MFMA inputs with fp32 accumulation,
// 2 (DEFAULT since round 3: the arithmetic bench.py's headline line runs) = fp32 as three bf16 planes, six products, 3 = nine products,
// 4 = fp32 as TWO fp16 planes, three products (conv_patch16.h: h2_split4) in the trunk's convolution kernels - the 3x3 forward / data
// gradient (conv_patch16_x3_kernel), the weight gradients (conv_wgrad_win16_kernel, conv_wgrad_x3_kernel, stem_wgrad_kernel), the stem's
// forward (conv_stem_patch_kernel) - wherever the caller names the operands' maxima (lmkd_conv_operand_amax); every other launch (the
// 1x1 forward, the inference epilogues, the loader-side BatchNorm), and every launch without them, runs mode 2.  Read through conv_nprod only.
static int g_conv_mode = 2;
static std::atomic<long> g_h2_launches{0};       // launches that took the two-plane form (tests; the forward's thread and the autograd engine's both launch)
static std::atomic<long> g_h2_fallbacks{0};      // mode-4 launches whose caller withheld a maximum because the range fence flagged the tensor (LMKD_AMAX_FENCED)
extern "C" long lmkd_conv_h2_launches(void) { return g_h2_launches.load(); }
extern "C" long lmkd_conv_h2_fallbacks(void) { return g_h2_fallbacks.load(); }
extern "C" int lmkd_conv_set_compute_dtype(int mode) {
  LMKD_REQUIRE(mode >= 0 && mode <= 4, "lmkd_conv_set_compute_dtype: 0 fp32 MFMA, 1 bf16, 2 fp32 as 3xbf16 (6 products), 3 (9 products), 4 fp32 as 2xfp16 (3 products) over mode 2");
  g_conv_mode = mode;
  return LMKD_OK;
}
extern "C" int lmkd_conv_get_compute_dtype(void) { return g_conv_mode; }
// MFMA products per fp32 product of a launch: 0 = the fp32 MFMA tile kernels (mode 0), 1 = one bf16 plane (mode 1; bf16 tensors, act16),
// 6 / 9 = three bf16 planes (modes 2 / 3), 3 = two fp16 planes: mode 4, for a launch that has that form and the operands' maxima (`maxima`).
// The only reader of the arithmetic mode.
static inline int conv_nprod(bool act16 = false, bool maxima = false) {
  if (act16) return 1;
  switch (g_conv_mode) {
    case 0: return 0;
    case 1: return 1;
    case 3: return 9;
    case 4: return maxima ? 3 : 6;
    default: return 6;
  }
}
static inline bool conv_planes() { return conv_nprod() != 0; }      // modes 1 - 4: weights as bf16 planes in fragment order (conv_x3.h)
static inline bool conv_h2() { return conv_nprod(false, true) == 3; }
static inline void note_fenced(const lmkd_amax_desc* am) { if (conv_h2() && am && (am->flags & LMKD_AMAX_FENCED)) ++g_h2_fallbacks; }
// The maxima of a launch's operands travel as explicit arguments (lmkd_amax_desc on the *_seg entry points; round 5 - before: one-shot
// thread-local channels).  x_words / dy_words: device words holding the fp32 bits of max |x| / max |dy| per frame segment (upper bounds are
// valid: a larger word costs range, not correctness), complete in stream order before the launch; either may be null; only mode 4 reads
// them.  out_words (forward): the launch also folds max |y| into these words - in the epilogue of conv_patch16_x3_kernel, or by a
// reduction pass of its own behind any other kernel - so that lmkd_bn_finalize_seg can bound relu(BatchNorm(y)) for a consumer that
// applies the BatchNorm in its loader.
// elements (16-bit) of the plane buffer of a packed weight of ncols x Kp in the current mode (wplanes.h)
extern "C" long lmkd_conv2d_plane_elems(int ncols, int Kp) { return wpl_total((long)ncols * Kp, g_conv_mode); }
// max |x| of n floats into the slot words of one frame segment of an activation maximum (lmkd_amax_next's layout: segment s at
// word + s * lmkd_amax_words() / 2).  The words are zeroed here first (zero).
static int amax_impl(const float* x, long n, void* word, void* stream, bool zero = true) {
  LMKD_REQUIRE(x && word && n > 0, "lmkd_amax: bad arguments");
  if (zero && hipMemsetAsync(word, 0, LMKD_AMAX_SEG_WORDS * 4, (hipStream_t)stream) != hipSuccess) {
    lmkd_set_error("lmkd_amax: hipMemsetAsync failed");
    return LMKD_EHIP;
  }
  int grid = cdiv(n, 256 * 16);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL(amax_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, (unsigned*)word);
  LMKD_CHECK_LAUNCH("amax_kernel");
  return LMKD_OK;
}
extern "C" int lmkd_amax(const float* x, long n, void* word, void* stream) { return amax_impl(x, n, word, stream); }

// The plane buffers of the m entries of a batch in the current arithmetic (modes 1 - 4; wplanes.h): gx workgroups per entry and pass
template <class E, int N>
static int wpl_write(WplBatch<E, N>& a, int m, int gx, void* stream) {
  using B = WplBatch<E, N>;
  a.npl = conv_nprod() == 1 ? 1 : 3;
  a.h2 = conv_h2();
  for (int j = 0; j < m; ++j) {
    const E& e = a.e[j];
    LMKD_REQUIRE(e.ncols > 0 && e.ncols % 32 == 0 && e.Kp > 0 && e.Kp % 32 == 0, "weight planes: entry %d: ncols=%d and Kp=%d must be multiples of 32", j, e.ncols, e.Kp);
    LMKD_REQUIRE(2 * wpl_total((long)e.ncols * e.Kp, 2) < 0xffffffe0L, "weight planes: entry %d: weights exceed the 4 GiB buffer range", j);
  }
  hipLaunchKernelGGL(wpl_bf16_kernel<B>, dim3(gx, m), dim3(256), 0, (hipStream_t)stream, a);
  LMKD_CHECK_LAUNCH("wpl_bf16_kernel");
  if (a.h2) {
    hipLaunchKernelGGL(wpl_amax_kernel<B>, dim3(std::min(gx, 512), m), dim3(256), 0, (hipStream_t)stream, a);      // (one atomic per wave on the entry's word: few workgroups)
    LMKD_CHECK_LAUNCH("wpl_amax_kernel");
    hipLaunchKernelGGL(wpl_h2_kernel<B>, dim3(gx, m), dim3(256), 0, (hipStream_t)stream, a);
    LMKD_CHECK_LAUNCH("wpl_h2_kernel");
  }
  return LMKD_OK;
}

extern "C" int lmkd_conv2d_split_weights(const float* wp, void* wf, int ncols, int Kp, void* stream) {
  LMKD_REQUIRE(wp && wf, "lmkd_conv2d_split_weights: null pointer");
  WplBatch<WplPacked, 1> a;
  a.e[0] = WplPacked{wp, (unsigned short*)wf, ncols, Kp};
  int grid = cdiv((long)ncols * Kp, 256);
  if (grid > 4096) grid = 4096;
  return wpl_write(a, 1, grid, stream);
}

// Re-pack MANY convolution weights in one launch per pass (after an optimizer step: 40 cached packs = 120 pack / split launches before).
// ws[i], wfs[i]: OIHW weight and destination planes of entry i; dims[i * 6 ..] = Cout, Cin, Cs, KH, KW, mode: what
// lmkd_conv2d_pack_weights + lmkd_conv2d_split_weights would write in the current arithmetic (modes 1 - 4), bit for bit.
#define LMKD_REPACK_MAX 40
extern "C" int lmkd_conv2d_repack_multi(const float* const* ws, void* const* wfs, const int* dims, int n, void* stream) {
  LMKD_REQUIRE(ws && wfs && dims && n > 0, "lmkd_conv2d_repack_multi: null pointer");
  LMKD_REQUIRE(conv_planes(), "lmkd_conv2d_repack_multi: fragment-order planes exist in the bf16-plane modes only");
  for (int i0 = 0; i0 < n; i0 += LMKD_REPACK_MAX) {
    WplBatch<WplOihw, LMKD_REPACK_MAX> a;
    memset(&a, 0, sizeof(a));
    const int m = std::min(LMKD_REPACK_MAX, n - i0);
    long most = 0;
    for (int j = 0; j < m; ++j) {
      const int* d = dims + (long)(i0 + j) * 6;
      LMKD_REQUIRE(ws[i0 + j] && wfs[i0 + j] && (d[5] == 0 || d[5] == 1), "lmkd_conv2d_repack_multi: bad entry %d", i0 + j);
      LMKD_REQUIRE(d[2] >= d[1] && (d[2] % 32 == 0 || d[2] == 4), "lmkd_conv2d_repack_multi: Cs=%d must be 4 or a multiple of 32", d[2]);
      a.e[j] = wpl_oihw(ws[i0 + j], wfs[i0 + j], d[0], d[1], d[2], d[3], d[4], d[5]);
      most = std::max(most, (long)a.e[j].ncols * a.e[j].Kp);
    }
    int gx = cdiv(most, 256 * 4);
    if (gx > 512) gx = 512;
    const int rc = wpl_write(a, m, gx, stream);
    if (rc) return rc;
  }
  return LMKD_OK;
}

// ---- tile configuration -------------------------------------------------------------------------
// id: 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 64x128 (rows x cols, 4 waves), 5 = 128x128 and 6 = 128x64 with 8 waves (2 per SIMD).
// Workgroups per CU by LDS: 2 / 2 / 4 / 2 / 2.
static int g_tile_override = 0;
extern "C" int lmkd_conv_set_tile(int id) {
  LMKD_REQUIRE(id >= 0 && id <= 14, "lmkd_conv_set_tile: id must be 0 (auto) .. 14");
  g_tile_override = id;
  return LMKD_OK;
}
// 7..10: the bf16-plane kernels (conv_x3.h, conv_patch.h), 8 waves: 7 = 256x64, 8 = 128x128, 9 = 128x64, 10 = 256x128 (patch kernel only)
// 11 / 12 (patch kernel only): 128x64 / 128x128 with FOUR waves, three / two workgroups per CU
// 13 / 14 (patch kernel, one-plane modes only): 256x128 / 256x64 with FOUR waves (wave tiles 128x64 / 128x32)
static inline int cfg_bm(int id) { return (id == 7 || id == 10 || id == 13 || id == 14) ? 256 : ((id <= 2 || id >= 5) ? 128 : 64); }
static inline int cfg_bn(int id) { return (id == 1 || id == 4 || id == 5 || id == 8 || id == 10 || id == 12 || id == 13) ? 128 : 64; }
static inline int cfg_wg_per_cu(int id) { return id == 1 ? 2 : (id == 3 ? 4 : 3); }

// Pick the tile that minimises ceil(tiles / 256 CUs) * work per tile: at 64 cycles per fp32 MFMA every configuration is
// matrix-pipe bound, so what differs is how evenly the launch's tiles divide over the CUs (the tail).
// same: same-size convolution served by the LDS-patch kernel (patch_eligible)
static int pick_conv_cfg(long rows_per_class, int nclass, int ncols, bool same = false) {
  if (conv_planes()) {
    if (g_tile_override >= 7) {
      int id = g_tile_override;
      if (id == 10 && !same) id = 8;
      if (id == 11 && !same) id = 9;
      if (id == 12 && !same) id = 8;
      if ((id == 13 || id == 14) && (!same || conv_nprod() != 1)) id = id == 13 ? 10 : 7;
      if (id == 10 && !same) id = 8;
      if (ncols <= 64 && cfg_bn(id) == 128) id = id == 10 ? 7 : (id == 12 ? 11 : (id == 13 ? 14 : 9));
      return id;
    }
    if (same) {
      // patch kernel, measured at 200 frames (tools/patch_bench.py): four-wave workgroups, two or three per CU, beat one eight-wave
      // workgroup - a workgroup's prologue / epilogue / chunk refill runs under the other workgroups' MFMAs.  128x128 (wave tile
      // 64x64: half the LDS reads per MFMA) in the three-plane modes once it gives every CU at least two rounds of tiles, 128x64 otherwise.
      if (ncols <= 64) return 11;
      const long t128 = cdiv(rows_per_class, 128) * cdiv(ncols, 128);
      return (conv_nprod() != 1 && t128 >= 1024) ? 12 : 11;      // one-plane modes: 128x64 throughout (three or four workgroups per CU)
    }
    if (ncols <= 64) return 9;
    // measured (tools/conv_bench_x3.py): 128x128 (one workgroup per CU) wins once the launch has a tile per CU
    return (long)nclass * cdiv(rows_per_class, 128) * cdiv(ncols, 128) >= 256 ? 8 : 9;
  }
  if (g_tile_override) {
    if (ncols <= 64 && cfg_bn(g_tile_override) == 128) return g_tile_override == 5 ? 6 : (cfg_bm(g_tile_override) == 128 ? 2 : 3);
    return g_tile_override;
  }
  int best = 0;
  double best_cost = 1e30;
  const int cand[4] = {5, 2, 4, 3};
  for (int c = 0; c < 4; ++c) {
    const int id = cand[c];
    if (ncols <= 64 && cfg_bn(id) == 128) continue;
    const long tiles = (long)nclass * cdiv(rows_per_class, cfg_bm(id)) * cdiv(ncols, cfg_bn(id));
    // matrix-pipe-bound model: a CU's time is the MFMA work of the tiles it receives, whatever their concurrency.
    // Measured per layer (profiles/): what matters is 4 waves per SIMD.  128x128 with 8 waves (2 workgroups per CU)
    // sustains 115-119 TFLOP/s when the launch has many tiles, 64x64 with 4 waves (4 per CU) 104-110, the 4-wave 128-wide
    // tiles (2 waves per SIMD) 92-103.
    double cost = (double)cdiv(tiles, 256) * cfg_bm(id) * cfg_bn(id);
    cost *= (id == 5 ? 0.92 : (id == 3 ? 1.00 : 1.07));
    // stride-2 data gradient: a parity class runs only 1-4 of the 9 taps, i.e. 4-64 K-steps per tile; the big tiles' longer
    // prologue / epilogue then dominates (measured, 200 frames: layer3.0.conv1 dgrad 79 TFLOP/s with 64x64 vs 59 with 128x128)
    if (nclass == 4 && id != 3) cost *= 1.5;
    if (cost < best_cost) { best_cost = cost; best = id; }
  }
  return best;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel instance, once per (instance, device), from whichever host thread launches
// first (the forward's thread and the autograd engine's both launch): `mask` is the instance's static bit set of devices done.
static inline void lmkd_lds_attr_once(std::atomic<unsigned long long>& mask, const void* fn, int bytes) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  const unsigned long long bit = 1ull << (d & 63);
  if (mask.load(std::memory_order_acquire) & bit) return;
  const hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (err != hipSuccess) {      // the launch that follows fails with its own message; leave the bit clear so that the next launch retries
    lmkd_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d): %s", bytes, hipGetErrorString(err));
    return;
  }
  mask.fetch_or(bit, std::memory_order_release);
}
template <auto K>
static inline void lds_attr_once(int bytes) {
  static std::atomic<unsigned long long> mask{0};
  lmkd_lds_attr_once(mask, reinterpret_cast<const void*>(K), bytes);
}

// Grid of a PERSISTENT launch (conv_patch.h): no more workgroups than the chip holds at once (occupancy of this instance with `lds` bytes of
// dynamic LDS x CUs), each walking `total` / grid slots of the tile order.  The grid is the smallest multiple of 8 that needs the same
// number of rounds as all resident slots would - every workgroup then has (nearly) the same number of tiles - and a multiple of 8 keeps a
// workgroup's slots on one XCD (xcd_decode: slot & 7).  The occupancy is asked once per (instance, LDS size).
struct PersistOcc { std::atomic<int> n{0}; int lds[8]; int occ[8]; std::mutex mu; };
static int lmkd_cu_count() {
  static std::atomic<int> n{0};
  int v = n.load(std::memory_order_relaxed);
  if (v) return v;
  int d = 0;
  hipDeviceProp_t pr;
  if (hipGetDevice(&d) != hipSuccess || hipGetDeviceProperties(&pr, d) != hipSuccess || pr.multiProcessorCount < 1) return 256;
  n.store(pr.multiProcessorCount, std::memory_order_relaxed);
  return pr.multiProcessorCount;
}
static int g_conv_persist = 1;      // 0: one workgroup per slot of the tile order (the form before round 5; for A/B measurements)
extern "C" int lmkd_conv_set_persistent(int on) { g_conv_persist = on ? 1 : 0; return LMKD_OK; }
template <auto K>
static int persistent_grid(int threads, size_t lds, int total) {
  if (!g_conv_persist) return total;
  static PersistOcc c;
  int occ = 0;
  {
    std::lock_guard<std::mutex> lk(c.mu);
    const int n = c.n.load();
    for (int i = 0; i < n; ++i) if (c.lds[i] == (int)lds) occ = c.occ[i];
    if (!occ) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, K, threads, lds) != hipSuccess || occ < 1) occ = 1;
      if (n < 8) { c.lds[n] = (int)lds; c.occ[n] = occ; c.n.store(n + 1); }
    }
  }
  const int slots = occ * lmkd_cu_count();
  if (total <= slots) return total;
  const int rounds = cdiv(total, slots);
  const int g = (cdiv(total, rounds) + 7) & ~7;
  return g < total ? g : total;
}

// Same-size convolutions (3x3 / stride 1 forward and data gradient, 1x1 / stride 1) of the bf16-plane modes read an LDS-resident
// input patch (conv_patch.h).  Returns the halo (largest |dh * Ws + dw| over the taps), or -1 when the launch is not of that kind.
static int g_conv_patch = 1;   // same-size convolutions of the bf16-plane modes from an LDS-resident patch (conv_patch.h); 0 = im2col gather
extern "C" int lmkd_conv_set_patch(int on) { g_conv_patch = on ? 1 : 0; return LMKD_OK; }
static int patch_halo(const ConvGemmArgs& a) {
  if (!g_conv_patch || !conv_planes() || a.Cs % 32 != 0 || a.sh != 1) return -1;
  // one class: output grid = input grid; four parity classes (stride-2 data gradient): each class runs on the dy grid
  const bool plain = a.nclass == 1 && a.Hs == a.Ho && a.Ws == a.Wo;
  const bool classes = a.nclass == 4 && a.Hr == a.Hs && a.Wr == a.Ws;
  if (!plain && !classes) return -1;
  int halo = 0;
  for (int c = 0; c < a.nclass; ++c)
    for (int t = 0; t < a.ntap[c]; ++t) {
      const int sft = a.taps[c][t].dh * a.Ws + a.taps[c][t].dw;
      halo = std::max(halo, sft < 0 ? -sft : sft);
    }
  return halo <= PATCH_HALO_MAX ? halo : -1;
}
static inline bool conv_same_size(int H, int W, int KH, int KW, int stride, int pad) {
  return g_conv_patch && stride == 1 && conv_out(H, KH, stride, pad) == H && conv_out(W, KW, stride, pad) == W && (KH / 2) * W + KW / 2 <= PATCH_HALO_MAX;
}

static int g_conv_s2_patch = 1;      // stride-2 3x3 forward on conv_patch16_x3_kernel's SRC2 form; 0 = im2col-gather kernel
extern "C" int lmkd_conv_set_s2_patch(int on) { g_conv_s2_patch = on ? 1 : 0; return LMKD_OK; }
// three-plane modes, fp32 tensors, the 4-wave tiles: conv_patch16_x3_kernel (v_mfma_f32_16x16x32_*); 0 = conv_patch_x3_kernel (32x32x16).
// 1 (default) = automatic: the 16x16x32 kernel, except the TWO-PLANE launches with Cout <= 64 (layer 1; NOT the 64-column tile of a wider layer: the
// two-call and the merged form of an episode pick different tiles there and must stay bit-identical), which run
// conv_patch_x3_kernel<.., 3, ..> on v_mfma_f32_32x32x16_f16 - with half the MFMAs of the three-plane form these launches are bound by
// vector-instruction issue (5.6 vector instructions per 16x16x32 MFMA, which holds the SIMD's vector issue for 8 of its 16 cycles; a
// 32x32x16 MFMA does the work of two and holds it for 8 of 32), and a lane of the 32x32 result owns ONE channel, so the BatchNorm sums
// need one shuffle instead of a 16-lane reduction per channel: 431 -> 350 us forward + sums, 378 -> 347 us data gradient at 400 frames
// (profiles/r05_patch32_vs_16.txt; the 128-column tiles of layers 2-4 stay 5-10 % faster on 16x16x32).  2 = 16x16x32 everywhere.
static int g_patch16 = 1;
extern "C" int lmkd_conv_set_patch16(int on) { g_patch16 = on < 0 ? 0 : (on > 2 ? 2 : on); return LMKD_OK; }

#ifdef LMKD_STAMPS
extern "C" int lmkd_debug_stamps(unsigned long long* host, int zero) {
  if (zero) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_lmkd_stamps)) != hipSuccess) return LMKD_EHIP;
    return hipMemset(p, 0, sizeof(g_lmkd_stamps)) == hipSuccess ? LMKD_OK : LMKD_EHIP;
  }
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_lmkd_stamps), sizeof(g_lmkd_stamps)) == hipSuccess ? LMKD_OK : LMKD_EHIP;
}
#endif
static inline int taps_within_one(const ConvGemmArgs& a) {
  for (int c = 0; c < a.nclass; ++c)
    for (int t = 0; t < a.ntap[c]; ++t)
      if (a.taps[c][t].dh < -1 || a.taps[c][t].dh > 1 || a.taps[c][t].dw < -1 || a.taps[c][t].dw > 1) return 0;
  return 1;
}

// stride-2 3x3 forward convolution as four same-size convolutions over the input's parity classes (conv_patch16.h, SRC2)?
static bool fwd_s2_patch_ok(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad) {
  if (!(g_conv_s2_patch && g_patch16 && g_conv_patch && conv_nprod(g_lmkd_act_bf16) >= 6) || Cs % 32 != 0 || stride != 2 || KH != 3 ||
      KW != 3 || pad != 1 || H % 2 != 0 || W % 2 != 0 || W / 2 + 1 > PATCH_HALO_MAX)
    return false;
  const int id = pick_conv_cfg((long)N * (H / 2) * (W / 2), 1, Cout, true);
  return id == 11 || id == 12;
}

// The stem (7x7 / stride 2 / pad 3 on the NHWC4 input, Cout <= 64) of the bf16-plane modes runs conv_stem_patch_kernel (conv_stem.h):
// one workgroup per pair of output rows.  Returns the patch row pitch in pixels, or 0 when the launch is not of that kind.
static int g_conv_stem_patch = 1;
extern "C" int lmkd_conv_set_stem_patch(int on) { g_conv_stem_patch = on ? 1 : 0; return LMKD_OK; }
static int stem_patch_pitch(int W, int Cs, int Cout, int KH, int KW, int stride, int pad) {
  if (!g_conv_stem_patch || !conv_planes() || Cs != 4 || KH != 7 || KW != 7 || stride != 2 || pad != 3 || Cout > 64) return 0;
  const int Wo = conv_out(W, KW, stride, pad);
  int wp = std::max(2 * Wo + 6, W + 3);
  wp += wp & 1;
  return (2 * Wo <= 256 && wp <= STEM_MAX_WP) ? wp : 0;
}

// ---- forward / data-gradient plan ------------------------------------------------------------------
// Which kernel instance a forward or data-gradient launch runs, with its tile order, grid and LDS: decided once, by plan_fwd / plan_dgrad,
// from the launch's arguments (shapes, frame segments, which operands are given), the switches and the arithmetic mode.  The launch
// (launch_conv), the report (lmkd_conv2d_plan) and the buffer sizes (lmkd_conv2d_fwd_row_tiles_seg, lmkd_conv2d_bwd_data_bn_tiles_seg)
// all read the same plan.
enum class ConvFam : unsigned char {
  Tile,       // fp32 MFMA tiles (conv_gemm_kernel), tile ids 1 - 6
  Gather,     // bf16-plane im2col gather (conv_gemm_x3_kernel), ids 7 / 8 / 9
  Patch,      // LDS-resident patch on the 32x32x16 MFMA (conv_patch_x3_kernel), ids 7 - 12; persistent in the two-plane form
  Patch16,    // LDS-resident patch on the 16x16x32 MFMA (conv_patch16_x3_kernel), ids 11 / 12: SRC2 / BNB / EP / PRE forms
  Patch1p,    // one-plane 256-row patch tiles (conv_patch_x3_kernel), ids 13 / 14
  Stem,       // the stem's input-row patch (conv_stem_patch_kernel), reported as id 14
};
// loader / epilogue of the launch: plain, BatchNorm + ReLU in the loader (PRE), inference BatchNorm epilogue (EP), bf16 tensors in HBM,
// the data gradient's BatchNorm-backward sums in the epilogue (BNB)
enum ConvIO : unsigned char { IO_PLAIN, IO_PRE, IO_EP, IO_ACT16, IO_BNB };
struct ConvPlan {
  ConvFam fam;
  unsigned char io;       // ConvIO
  bool src2;              // Patch16: the stride-2 forward over the input's four parity classes
  bool smallc;            // Tile / Gather: the padded stem input (Cs = 4)
  bool bnb_form;          // data gradient: the launch has the fused BatchNorm-backward form (lmkd_conv2d_bwd_data_bn_tiles_seg)
  bool amax_pass;         // max |y| (ConvGemmArgs::amax_out) needs a reduction pass behind the kernel: its epilogue does not fold it
  int stats;              // Tile: conv_gemm_kernel STATS
  int tile;               // lmkd_conv_set_tile id
  int nprod;              // conv_nprod of the launch
  int nclass, xcd;        // parity classes, XCD tile order (xcd_decode)
  int halo;               // patch kernels: ConvGemmArgs::halo; Stem: the patch row pitch
  int seg_m0, seg_t0, tiles_per_class, n_rt, n_ct;      // row tiles of the launch (conv_set_tiles): segment 0 has seg_t0 of each class's
  int grid;               // workgroups; persistent launches: slots of the tile order (the grid then comes from the occupancy at launch)
  int lds;                // dynamic LDS bytes
};

// geometry of a forward launch (no operands).  Taps are filled only where they fit (a report may ask for shapes no launch takes).
static void fwd_geometry(ConvGemmArgs& a, int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, int seg_n0) {
  memset(&a, 0, sizeof(a));
  const int KWp = kw_padded(Cs, KW);
  a.N = N; a.Hs = H; a.Ws = W; a.Cs = Cs;
  a.Ho = conv_out(H, KH, stride, pad); a.Wo = conv_out(W, KW, stride, pad); a.Co = Cout;
  a.Hr = a.Ho; a.Wr = a.Wo; a.rows_per_class = N * a.Ho * a.Wo; a.tiles_per_class = cdiv(a.rows_per_class, 128);
  a.seg_m0 = seg_n0 * a.Ho * a.Wo;      // 0: one segment (conv_set_tiles)
  a.sh = stride; a.omul = 1; a.nclass = 1;
  a.Kp = KH * KWp * Cs;
  a.div_hw = make_fastdiv(a.Hr * a.Wr); a.div_w = make_fastdiv(a.Wr);
  if (Cs == 4) {
    a.cps = 1;
    if (KH > LMKD_MAX_TAPS) return;
    a.ntap[0] = KH;
    for (int kh = 0; kh < KH; ++kh) a.taps[0][kh] = Tap{kh - pad, -pad, kh * KWp * Cs};
  } else {
    a.cps = Cs / 32;
    if (KH * KW > LMKD_MAX_TAPS) return;
    a.ntap[0] = KH * KW;
    for (int kh = 0; kh < KH; ++kh)
      for (int kw = 0; kw < KW; ++kw) a.taps[0][kh * KW + kw] = Tap{kh - pad, kw - pad, (kh * KWp + kw) * Cs};
  }
}

// geometry of a data-gradient launch dx[N,H,W,Cin] from dy[N,Ho,Wo,Cout] (no operands; taps only where they fit)
static void dgrad_geometry(ConvGemmArgs& a, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int seg_n0) {
  memset(&a, 0, sizeof(a));
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  a.N = N; a.Hs = Ho; a.Ws = Wo; a.Cs = Cout;
  a.Ho = H; a.Wo = W; a.Co = Cin;
  a.Kp = KH * KW * Cout; a.cps = Cout / 32;
  a.sh = 1;
  const bool fits = KH * KW <= LMKD_MAX_TAPS;
  if (stride == 1) {
    a.nclass = 1; a.omul = 1; a.Hr = H; a.Wr = W;
    int nt = 0;
    for (int kh = 0; kh < KH && fits; ++kh)
      for (int kw = 0; kw < KW; ++kw) a.taps[0][nt++] = Tap{pad - kh, pad - kw, (kh * KW + kw) * Cout};
    a.ntap[0] = nt;
  } else {
    // rows enumerated per input parity (ph,pw): ih = 2a+ph, source oh = (ih + pad - kh)/2 = a + (ph+pad-kh)/2
    a.nclass = 4; a.omul = 2; a.Hr = (H + 1) / 2; a.Wr = (W + 1) / 2;
    for (int c = 0; c < 4 && fits; ++c) {
      const int ph = c >> 1, pw = c & 1;
      int nt = 0;
      for (int kh = 0; kh < KH; ++kh) {
        if (((ph + pad - kh) & 1) != 0) continue;
        for (int kw = 0; kw < KW; ++kw) {
          if (((pw + pad - kw) & 1) != 0) continue;
          // floor division (numerator may be negative)
          const int nh = ph + pad - kh, nw = pw + pad - kw;
          a.taps[c][nt++] = Tap{nh >= 0 ? nh / 2 : -((-nh) / 2), nw >= 0 ? nw / 2 : -((-nw) / 2), (kh * KW + kw) * Cout};
        }
      }
      a.ntap[c] = nt;
    }
  }
  a.rows_per_class = N * a.Hr * a.Wr;
  a.seg_m0 = seg_n0 * a.Hr * a.Wr;
  a.tiles_per_class = cdiv(a.rows_per_class, 128);
  a.div_hw = make_fastdiv(a.Hr * a.Wr); a.div_w = make_fastdiv(a.Wr);
}

// The kernel choice of every forward / data-gradient launch but the stem's.  halo: patch_halo of the launch (-1: not a patch launch);
// same: same-size convolution (the tile may be one only the patch kernel has); src2: the stride-2 forward's parity-class form.
static ConvPlan plan_conv(const ConvGemmArgs& a, int halo, bool same, bool smallc, int stats, bool src2) {
  ConvPlan p;
  memset(&p, 0, sizeof(p));
  const bool act16 = g_lmkd_act_bf16;
  const int ncols = a.Co;
  p.io = a.ep_stats ? IO_EP : act16 ? IO_ACT16 : a.pre_stats ? IO_PRE : a.bnb_x ? IO_BNB : IO_PLAIN;
  p.src2 = src2; p.smallc = smallc; p.stats = stats; p.nclass = a.nclass; p.halo = halo;
  int id = pick_conv_cfg(a.rows_per_class, a.nclass, ncols, same);
  // (the inference epilogue of the padded stem input exists on the fp32 tiles only)
  if (conv_planes() && !(stats == 2 && smallc)) {
    if (halo < 0) {      // the gather kernel: the same tile height (the BatchNorm partials' row count) where the patch kernel's tile was picked
      id = id == 10 || id == 13 || id == 14 ? 7 : (id == 11 ? 9 : (id == 12 ? 8 : id));
      p.fam = ConvFam::Gather;
      p.nprod = conv_nprod(act16);
    } else if (id == 13 || id == 14) {
      p.fam = ConvFam::Patch1p;
      p.nprod = 1;
    } else {
      const bool h2 = conv_nprod(act16, a.h2_xw && !a.ep_stats) == 3;      // two fp16 planes (not the inference epilogue)
      const bool h2_on_32 = g_patch16 == 1 && id == 11 && ncols <= 64 && h2 && !src2;
      const bool p16 = (id == 11 || id == 12) && g_patch16 && conv_nprod(act16) >= 6;
      // the fused BatchNorm-backward sums: conv_patch16_x3_kernel's one-class launches (BNB), or the two-plane form on 32x32x16
      // (h2_on_32), whose epilogue takes them as well
      p.bnb_form = p16 && a.nclass == 1 && ncols % 4 == 0;
      if (p16 && !h2_on_32) {
        p.fam = ConvFam::Patch16;
        p.nprod = conv_nprod(false, a.h2_xw);      // (the inference epilogue too)
      } else {
        p.fam = ConvFam::Patch;
        p.nprod = h2 ? 3 : conv_nprod(act16);
      }
    }
  } else {
    p.fam = ConvFam::Tile;
    if (id != 1 && id != 2 && id != 3 && id != 5 && id != 6) id = 4;
  }
  p.tile = id;
  // row tiles, per frame segment (conv_set_tiles)
  const int bm = cfg_bm(id);
  p.seg_m0 = (a.seg_m0 <= 0 || a.seg_m0 >= a.rows_per_class) ? a.rows_per_class : a.seg_m0;
  p.seg_t0 = cdiv(p.seg_m0, bm);
  p.tiles_per_class = p.seg_t0 + cdiv(a.rows_per_class - p.seg_m0, bm);
  p.n_rt = a.nclass * p.tiles_per_class;
  p.n_ct = cdiv(ncols, cfg_bn(id));
  p.xcd = g_xcd_mode != 0 && p.n_ct >= 8 && (p.n_ct & 7) == 0;
  p.grid = xcd_grid(p.n_rt, p.n_ct, p.xcd);
  if (p.fam == ConvFam::Patch || p.fam == ConvFam::Patch16 || p.fam == ConvFam::Patch1p)
    p.lds = (int)patch_lds_bytes(bm, halo, p.nprod == 1 ? 1 : (p.nprod == 3 && p.fam == ConvFam::Patch ? 2 : 3));
  // (x3_epilogue<.., H2> and conv_patch16_x3_kernel fold max |y| themselves)
  p.amax_pass = !act16 && p.fam != ConvFam::Patch16 && !(p.fam == ConvFam::Patch && p.nprod == 3);
  return p;
}

// a: fwd_geometry (+ the operands; only whether they are given is read)
static ConvPlan plan_fwd(const ConvGemmArgs& a, int KH, int KW, int pad) {
  const int N = a.N, H = a.Hs, W = a.Ws, Cs = a.Cs, Cout = a.Co, stride = a.sh;
  if (const int wp = a.ep_stats ? 0 : stem_patch_pitch(W, Cs, Cout, KH, KW, stride, pad)) {      // one workgroup per output row pair
    ConvPlan p;
    memset(&p, 0, sizeof(p));
    p.fam = ConvFam::Stem;
    p.io = g_lmkd_act_bf16 ? IO_ACT16 : IO_PLAIN;
    p.tile = 14; p.nclass = 1; p.halo = wp;
    p.nprod = conv_nprod(g_lmkd_act_bf16, a.h2_xw);
    const int seg_n0 = a.seg_m0 > 0 && a.seg_m0 < a.rows_per_class ? a.seg_m0 / (a.Ho * a.Wo) : N;
    p.seg_t0 = seg_n0 * cdiv(a.Ho, 2);
    p.n_rt = p.tiles_per_class = p.grid = N * cdiv(a.Ho, 2);
    p.n_ct = 1;
    p.lds = (p.nprod == 1 ? 1 : 3) * 9 * wp * 8;
    return p;      // (no max |y| pass behind the stem)
  }
  const int stats = a.ep_stats ? 2 : (a.stat_partial ? 1 : 0);
  // stride-2 3x3 forward on the patch kernel (SRC2): even input, the 16x16x32 instances (tile ids 11 / 12), no BatchNorm loader.  Its
  // taps lie within -1 .. 0 of the class grid (= the output grid): halo Wo + 1
  if (!a.pre_stats && fwd_s2_patch_ok(N, H, W, Cs, Cout, KH, KW, stride, pad)) return plan_conv(a, a.Wo + 1, true, false, stats, true);
  const int halo = Cs == 4 || !a.ntap[0] ? -1 : patch_halo(a);
  return plan_conv(a, halo, conv_same_size(H, W, KH, KW, stride, pad), Cs == 4, stats, false);
}

// a: dgrad_geometry (+ the operands)
static ConvPlan plan_dgrad(const ConvGemmArgs& a) {
  const int halo = a.ntap[0] ? patch_halo(a) : -1;
  return plan_conv(a, halo, halo >= 0, false, 0, false);
}

// The stride-2 forward's parity-class form of the arguments (ConvGemmArgs::src2)
static void fwd_src2_args(ConvGemmArgs& a, int W, int KWp) {
  const int Cs = a.Cs;
  a.src2 = 1; a.s2_ncls = 4; a.s2_wfull = W;
  a.Hs = a.Ho; a.Ws = a.Wo; a.sh = 1;
  static const int order[4][2] = {{1, 1}, {1, 0}, {0, 1}, {0, 0}};      // classes by tap count 4, 2, 2, 1
  int nt = 0;
  for (int c = 0; c < 4; ++c) {
    const int sph = order[c][0], spw = order[c][1];
    a.s2_t0[c] = nt;
    a.s2_off[c] = (sph * W + spw) * Cs;
    for (int kh = 0; kh < 3; ++kh) {
      if (((kh - 1) & 1) != sph) continue;
      for (int kw = 0; kw < 3; ++kw) {
        if (((kw - 1) & 1) != spw) continue;
        a.taps[0][nt++] = Tap{(kh - 1 - sph) / 2, (kw - 1 - spw) / 2, (kh * KWp + kw) * Cs};
      }
    }
  }
  a.s2_t0[4] = nt;
  a.ntap[0] = nt;
}

// ---- launching a plan ------------------------------------------------------------------------------
// f(std::integral_constant<int, P>{}) for the plan's product count n, P one of the counts the call site lists: a site instantiates
// exactly the instances it names.  Every two-plane launch passes through here (lmkd_conv_h2_launches).
template <int... Ps, class F>
static inline void with_nprod(int n, F&& f) {
  if (n == 3) ++g_h2_launches;
  (void)((n == Ps ? (f(std::integral_constant<int, Ps>{}), true) : false) || ...);
}

template <class Cfg, int NPROD, bool PRE, int IO>
static void launch_patch_instance(ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  constexpr auto K = conv_patch_x3_kernel<Cfg, NPROD, PRE, IO>;
  lds_attr_once<K>((int)patch_lds_bytes(Cfg::BM, PATCH_HALO_MAX, NPROD == 1 ? 1 : 3));
  a.grid_total = p.grid;      // (one-plane / three-plane instances: one workgroup per tile, conv_patch.h PERSIST)
  a.grid_step = NPROD == 3 ? persistent_grid<K>(Cfg::THREADS, p.lds, p.grid) : p.grid;
  hipLaunchKernelGGL((conv_patch_x3_kernel<Cfg, NPROD, PRE, IO>), dim3(a.grid_step), dim3(Cfg::THREADS), p.lds, s, a);
}
// conv_patch_x3_kernel (Patch, Patch1p)
template <class Cfg, bool ONE_PLANE = false>
static void launch_patch(ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  if constexpr (ONE_PLANE) {
    if (p.io == IO_EP) launch_patch_instance<Cfg, 1, false, 4>(a, p, s);
    else if (p.io == IO_ACT16) launch_patch_instance<Cfg, 1, false, 3>(a, p, s);
    else if (p.io == IO_PRE) launch_patch_instance<Cfg, 1, true, 0>(a, p, s);
    else launch_patch_instance<Cfg, 1, false, 0>(a, p, s);
  } else {
    if (p.io == IO_EP) with_nprod<1, 6, 9>(p.nprod, [&](auto np) { launch_patch_instance<Cfg, np, false, 4>(a, p, s); });
    else if (p.io == IO_ACT16) launch_patch_instance<Cfg, 1, false, 3>(a, p, s);
    else if (p.io == IO_PRE) with_nprod<1, 3, 6, 9>(p.nprod, [&](auto np) { launch_patch_instance<Cfg, np, true, 0>(a, p, s); });
    else with_nprod<1, 3, 6, 9>(p.nprod, [&](auto np) { launch_patch_instance<Cfg, np, false, 0>(a, p, s); });
  }
}
template <class Cfg, int NPROD, bool PRE, bool EP, bool SRC2 = false, bool BNB = false>
static void launch_patch16_instance(const ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  lds_attr_once<conv_patch16_x3_kernel<Cfg, NPROD, PRE, EP, SRC2, BNB>>((int)patch_lds_bytes(Cfg::BM, PATCH_HALO_MAX, 3));
  hipLaunchKernelGGL((conv_patch16_x3_kernel<Cfg, NPROD, PRE, EP, SRC2, BNB>), dim3(p.grid), dim3(Cfg::THREADS), p.lds, s, a);
}
// conv_patch16_x3_kernel (Patch16; the benchmark's tiles 11 / 12)
template <class Cfg>
static void launch_patch16(const ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  with_nprod<3, 6, 9>(p.nprod, [&](auto np) {
    if (p.src2 && p.io == IO_EP) launch_patch16_instance<Cfg, np, false, true, true>(a, p, s);      // inference, stride 2
    else if (p.src2) launch_patch16_instance<Cfg, np, false, false, true>(a, p, s);
    else if (p.io == IO_EP) launch_patch16_instance<Cfg, np, false, true>(a, p, s);      // BatchNorm affine (+ residual, ReLU)
    else if (p.io == IO_PRE) launch_patch16_instance<Cfg, np, true, false>(a, p, s);
    else if (p.io == IO_BNB) launch_patch16_instance<Cfg, np, false, false, false, true>(a, p, s);
    else launch_patch16_instance<Cfg, np, false, false>(a, p, s);
  });
}
// conv_gemm_x3_kernel (Gather).  ONE instance serves launches with and without BatchNorm partials (stat_partial null -> nothing written):
// hipcc schedules the main loop of the instance without the statistics epilogue worse (register copies in front of the MFMAs: 105 vs
// 148 TFLOP/s on the same layer), so that instance is not built
template <class Cfg, bool SMALLC>
static void launch_gather(const ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  const dim3 grid(p.grid), block(Cfg::THREADS);
  if (p.io == IO_ACT16) {      // bf16 tensors in HBM (one-plane mode): the loader copies, the epilogue rounds; the stem input stays fp32
    if constexpr (SMALLC) hipLaunchKernelGGL((conv_gemm_x3_kernel<Cfg, true, true, 1, false, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_gemm_x3_kernel<Cfg, false, true, 1, false, 3>), grid, block, 0, s, a);
    return;
  }
  if constexpr (!SMALLC) {
    if (p.io == IO_EP) {      // inference epilogue (x3_epilogue EP): stride-2 / 1x1-downsample convolutions of an eval forward
      with_nprod<1, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_gemm_x3_kernel<Cfg, false, true, np, false, 4>), grid, block, 0, s, a); });
      return;
    }
    if (p.io == IO_PRE) {      // training forward fed by relu(BatchNorm(raw)): normalise + rectify when the tile is stored to LDS
      with_nprod<1, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_gemm_x3_kernel<Cfg, false, true, np, true>), grid, block, 0, s, a); });
      return;
    }
  }
  with_nprod<1, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_gemm_x3_kernel<Cfg, SMALLC, true, np>), grid, block, 0, s, a); });
}
// conv_gemm_kernel (Tile)
template <class Cfg>
static void launch_tile(const ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  const dim3 grid(p.grid), block(Cfg::THREADS);
  if (p.smallc) {
    if (p.stats == 2) hipLaunchKernelGGL((conv_gemm_kernel<Cfg, true, 2, false>), grid, block, 0, s, a);
    else if (p.stats == 1) hipLaunchKernelGGL((conv_gemm_kernel<Cfg, true, 1, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_gemm_kernel<Cfg, true, 0, false>), grid, block, 0, s, a);
  } else if (p.stats == 2) hipLaunchKernelGGL((conv_gemm_kernel<Cfg, false, 2, false>), grid, block, 0, s, a);
  else if (p.stats == 1 && p.io == IO_PRE)      // the training forward of a conv that follows a BatchNorm + ReLU
    hipLaunchKernelGGL((conv_gemm_kernel<Cfg, false, 1, false, true>), grid, block, 0, s, a);
  else if (p.stats == 1) hipLaunchKernelGGL((conv_gemm_kernel<Cfg, false, 1, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv_gemm_kernel<Cfg, false, 0, false>), grid, block, 0, s, a);
}

// (round 4: conv_patch16_x3_kernel on 256 x 64 tiles - four waves stacked over the rows, wave tiles 64 x 64, two workgroups per CU - was
// built as tile id 15 and measured SLOWER than id 11 on every layer, 443 vs 383 us on layer 1 in fp32h2: profiles/r04_tile_ab.txt; removed)
static int launch_conv(ConvGemmArgs& a, const ConvPlan& p, hipStream_t s) {
  if (p.fam == ConvFam::Stem) {
    a.halo = p.halo;      // row pitch of the input-row patch
    a.n_rt = p.n_rt; a.n_ct = 1;
    const dim3 grid(p.grid), block(512);
    // two output rows per workgroup (one row, four waves: 557 vs 447 us at 200 frames)
    if (p.io == IO_ACT16) hipLaunchKernelGGL((conv_stem_patch_kernel<1, true, 2>), grid, block, p.lds, s, a);
    else with_nprod<1, 3, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_stem_patch_kernel<np, false, 2>), grid, block, p.lds, s, a); });
    LMKD_CHECK_LAUNCH("conv_stem_patch_kernel");
    return LMKD_OK;
  }
  a.seg_m0 = p.seg_m0; a.seg_t0 = p.seg_t0; a.tiles_per_class = p.tiles_per_class;
  a.n_rt = p.n_rt; a.n_ct = p.n_ct; a.xcd_mode = p.xcd;
  switch (p.fam) {
    case ConvFam::Tile:
      switch (p.tile) {
        case 1: launch_tile<TileCfg<128, 128, 2, 2>>(a, p, s); break;
        case 2: launch_tile<TileCfg<128, 64, 2, 2>>(a, p, s); break;
        case 3: launch_tile<TileCfg<64, 64, 2, 2>>(a, p, s); break;
        case 5: launch_tile<TileCfg<128, 128, 2, 4>>(a, p, s); break;
        case 6: launch_tile<TileCfg<128, 64, 4, 2>>(a, p, s); break;
        default: launch_tile<TileCfg<64, 128, 2, 2>>(a, p, s); break;
      }
      LMKD_CHECK_LAUNCH("conv_gemm_kernel");
      return LMKD_OK;
    case ConvFam::Gather:
      switch (p.tile * 2 + p.smallc) {
        case 14: launch_gather<X3Cfg<256, 64, 4, 2>, false>(a, p, s); break;
        case 15: launch_gather<X3Cfg<256, 64, 4, 2>, true>(a, p, s); break;
        case 16: launch_gather<X3Cfg<128, 128, 2, 4>, false>(a, p, s); break;
        case 17: launch_gather<X3Cfg<128, 128, 2, 4>, true>(a, p, s); break;
        case 19: launch_gather<X3Cfg<128, 64, 4, 2>, true>(a, p, s); break;
        default: launch_gather<X3Cfg<128, 64, 4, 2>, false>(a, p, s); break;
      }
      LMKD_CHECK_LAUNCH("conv_gemm_x3_kernel");
      return LMKD_OK;
    default: break;
  }
  a.taps_pm1 = taps_within_one(a);
  a.halo = p.halo;
  switch (p.tile) {
    case 7: launch_patch<X3Cfg<256, 64, 4, 2>>(a, p, s); break;
    case 8: launch_patch<X3Cfg<128, 128, 2, 4>>(a, p, s); break;
    case 10: launch_patch<X3Cfg<256, 128, 2, 4>>(a, p, s); break;
    case 11:
      if (p.fam == ConvFam::Patch16) launch_patch16<X3Cfg<128, 64, 2, 2, 3>>(a, p, s);
      else launch_patch<X3Cfg<128, 64, 2, 2, 3>>(a, p, s);
      break;
    case 12:
      if (p.fam == ConvFam::Patch16) launch_patch16<X3Cfg<128, 128, 2, 2, 2>>(a, p, s);
      else launch_patch<X3Cfg<128, 128, 2, 2, 2>>(a, p, s);
      break;
    case 13: launch_patch<X3Cfg<256, 128, 2, 2, 2>, true>(a, p, s); break;      // (one-plane modes only: 256-row tiles with four waves)
    case 14: launch_patch<X3Cfg<256, 64, 2, 2, 2>, true>(a, p, s); break;
    default: launch_patch<X3Cfg<128, 64, 4, 2>>(a, p, s); break;
  }
  LMKD_CHECK_LAUNCH("conv_patch_x3_kernel");
  return LMKD_OK;
}

// number of row tiles (= rows of the BN partial-statistics buffer) of a forward conv
extern "C" int lmkd_conv2d_fwd_row_tiles_seg(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, int seg_n0, int* tiles0);
extern "C" int lmkd_conv2d_fwd_row_tiles_cs(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad) {
  return lmkd_conv2d_fwd_row_tiles_seg(N, H, W, Cs, Cout, KH, KW, stride, pad, 0, nullptr);
}
// two frame segments in one launch (ConvGemmArgs::seg_m0): frames [0, seg_n0) | [seg_n0, N).  Returns the rows of the partial-sum
// buffer; *tiles0 (host pointer, nullable) receives how many of them - the leading ones - belong to segment 0.  seg_n0 = 0 or N: one segment.
extern "C" int lmkd_conv2d_fwd_row_tiles_seg(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, int seg_n0, int* tiles0) {
  if (seg_n0 <= 0 || seg_n0 >= N) seg_n0 = 0;
  ConvGemmArgs a;
  fwd_geometry(a, N, H, W, Cs, Cout, KH, KW, stride, pad, seg_n0);
  const ConvPlan p = plan_fwd(a, KH, KW, pad);
  if (tiles0) *tiles0 = p.seg_t0;
  return p.tiles_per_class;
}
extern "C" int lmkd_conv2d_fwd_row_tiles(int N, int H, int W, int Cout, int KH, int KW, int stride, int pad) {
  return lmkd_conv2d_fwd_row_tiles_cs(N, H, W, 32, Cout, KH, KW, stride, pad);
}

static int conv2d_fwd_impl(const float* x, const float* wp, float* y, float* stat_partial, const float* ep_stats,
                           const float* ep_res, int ep_relu, int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride,
                           int pad, void* stream, const float* pre_stats = nullptr, int seg_n0 = 0, const lmkd_amax_desc* am = nullptr) {
  LMKD_REQUIRE(x && wp && y, "lmkd_conv2d_fwd: null pointer");
  if (seg_n0 <= 0 || seg_n0 >= N) seg_n0 = 0;
  LMKD_REQUIRE(!seg_n0 || (conv_planes() && !ep_stats), "lmkd_conv2d_fwd_seg: two frame segments exist in the bf16-plane modes (training / plain forward)");
  LMKD_REQUIRE(aligned16(x) && aligned16(wp), "lmkd_conv2d_fwd: x / packed weights must be 16-byte aligned");
  LMKD_REQUIRE(Cs % 32 == 0 || Cs == 4, "lmkd_conv2d_fwd: channel count %d must be 4 (padded stem) or a multiple of 32", Cs);
  LMKD_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0, "lmkd_conv2d_fwd: empty tensor");
  const bool smallc = Cs == 4;
  const int KWp = kw_padded(Cs, KW);
  LMKD_REQUIRE(!smallc || KWp == 8, "lmkd_conv2d_fwd: padded-stem path needs KW <= 8");
  LMKD_REQUIRE(KH * (smallc ? 1 : KW) <= LMKD_MAX_TAPS, "lmkd_conv2d_fwd: kernel %dx%d has too many taps", KH, KW);
  LMKD_REQUIRE(H < 32768 && W < 32768, "lmkd_conv2d_fwd: spatial dims too large");
  const bool act16 = g_lmkd_act_bf16;
  LMKD_REQUIRE(!pre_stats || (stat_partial && !smallc && !act16),
               "lmkd_conv2d_fwd_pre: the fused BatchNorm+ReLU loader exists for the training forward with fp32 activations (stat_partial given, Cs %% 32 == 0)");
  LMKD_REQUIRE(!act16 || (conv_nprod() == 1 && !ep_stats), "bf16 activations need lmkd_conv_set_compute_dtype(1) (training / plain forward)");
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  LMKD_REQUIRE(Ho > 0 && Wo > 0, "lmkd_conv2d_fwd: empty output");
  LMKD_REQUIRE((long)N * H * W * Cs < 2147483647L && (long)N * Ho * Wo * Cout < 2147483647L,
               "lmkd_conv2d_fwd: tensor exceeds 2^31 elements");
  // the bf16-plane kernels (patch / stem / gather) address the gathered tensor with 32-bit BYTE offsets through a buffer resource
  LMKD_REQUIRE(!conv_planes() || (long)N * H * W * Cs * (act16 && Cs != 4 ? 2 : 4) < 0xffffffe0L,
               "lmkd_conv2d_fwd: input tensor exceeds the 4 GiB buffer range of the bf16-plane kernels");
  ConvGemmArgs a;
  fwd_geometry(a, N, H, W, Cs, Cout, KH, KW, stride, pad, seg_n0);
  a.src = x; a.wpk = wp; a.out = y; a.stat_partial = stat_partial;
  a.h2_xw = am ? (const unsigned*)am->x_words : nullptr;
  a.amax_out = am ? (unsigned*)am->out_words : nullptr;
  note_fenced(am);
  a.ep_stats = ep_stats; a.ep_res = ep_res; a.ep_relu = ep_relu;
  a.pre_stats = pre_stats;
  const ConvPlan p = plan_fwd(a, KH, KW, pad);
  if (p.src2) {
    LMKD_REQUIRE((long)N * H * W * Cs * 4 < 2147483647L, "lmkd_conv2d_fwd: input tensor exceeds the 2 GiB offset range of the stride-2 patch form");
    fwd_src2_args(a, W, KWp);
  }
  int rc = launch_conv(a, p, (hipStream_t)stream);
  if (rc == LMKD_OK && a.amax_out && p.amax_pass) {
    // lmkd_conv_output_amax on a launch whose kernel does not fold the maximum in its epilogue: a reduction pass of its own per frame
    // segment (rare shapes; the trunk's 3x3 convolutions all run conv_patch16_x3_kernel) - the words are never left at "unknown"
    const long per = (long)Ho * Wo * Cout, n0 = seg_n0 ? seg_n0 * per : (long)N * per;
    rc = amax_impl(y, n0, a.amax_out, stream, false);
    if (rc == LMKD_OK && seg_n0) rc = amax_impl(y + n0, (long)N * per - n0, a.amax_out + LMKD_AMAX_SEG_WORDS, stream, false);
  }
  return rc;
}

extern "C" int lmkd_conv2d_fwd(const float* x, const float* wp, float* y, float* stat_partial, int N, int H, int W, int Cs,
                               int Cout, int KH, int KW, int stride, int pad, void* stream) {
  return conv2d_fwd_impl(x, wp, y, stat_partial, nullptr, nullptr, 0, N, H, W, Cs, Cout, KH, KW, stride, pad, stream);
}

// Training form for a convolution that consumes relu(BatchNorm(x)): x_raw is the previous convolution's raw output and
// pre_stats its [5][Cs] BatchNorm table (lmkd_bn_finalize); normalise + ReLU happen in the loader, bit-identical to running
// lmkd_bn_apply first (torchvision BasicBlock: conv2(relu(bn1(conv1(x)))), resnet18_2fc.py:41-42).
// lmkd_conv2d_fwd / lmkd_conv2d_fwd_pre (pre_stats nullable) over TWO frame segments [0, seg_n0) | [seg_n0, N) of one tensor - the support-
// frame and the query-frame trunk call of an episode (resnet18_2fc.py:41-42) in one launch: pre_stats is a [2][5][Cs] table (one per
// segment), stat_partial has lmkd_conv2d_fwd_row_tiles_seg rows of which the first *tiles0 belong to segment 0.  Results are bit-identical
// to two launches on the two halves.  bf16-plane modes (lmkd_conv_set_compute_dtype 1-3).
extern "C" int lmkd_conv2d_fwd_seg(const float* x, const float* pre_stats, const float* wp, float* y, float* stat_partial, int N, int H, int W,
                                   int Cs, int Cout, int KH, int KW, int stride, int pad, int seg_n0, void* stream, const lmkd_amax_desc* amax) {
  return conv2d_fwd_impl(x, wp, y, stat_partial, nullptr, nullptr, 0, N, H, W, Cs, Cout, KH, KW, stride, pad, stream, pre_stats, seg_n0, amax);
}

extern "C" int lmkd_conv2d_fwd_pre(const float* x_raw, const float* pre_stats, const float* wp, float* y, float* stat_partial, int N,
                                   int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, void* stream) {
  LMKD_REQUIRE(pre_stats, "lmkd_conv2d_fwd_pre: BatchNorm table of the input missing");
  return conv2d_fwd_impl(x_raw, wp, y, stat_partial, nullptr, nullptr, 0, N, H, W, Cs, Cout, KH, KW, stride, pad, stream, pre_stats);
}

// Inference form: y = relu?( conv(x) * scale[c] + shift[c] (+ res) ) in the convolution's epilogue (scale/shift = rows 2/3 of
// the [5][C] table of lmkd_bn_eval_stats); the same operations in the same order as lmkd_conv2d_fwd + lmkd_bn_apply.
extern "C" int lmkd_conv2d_fwd_bn(const float* x, const float* wp, float* y, const float* bn_stats, const float* res, int relu,
                                  int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, void* stream, const lmkd_amax_desc* amax) {
  LMKD_REQUIRE(bn_stats, "lmkd_conv2d_fwd_bn: BatchNorm table missing");
  LMKD_REQUIRE(!g_lmkd_act_bf16, "lmkd_conv2d_fwd_bn: fp32 tensors only (with bf16 tensors run lmkd_conv2d_fwd + lmkd_bn_apply)");
  LMKD_REQUIRE(!conv_planes() || Cs % 32 == 0, "lmkd_conv2d_fwd_bn: the bf16-plane modes need Cs %% 32 == 0 (Cs=%d)", Cs);
  return conv2d_fwd_impl(x, wp, y, nullptr, bn_stats, res, relu, N, H, W, Cs, Cout, KH, KW, stride, pad, stream, nullptr, 0, amax);
}

// dx[N,H,W,Cin] (+= when accumulate) from dy[N,Ho,Wo,Cout]; wd = weights packed with mode 1
static int bwd_data_args(ConvGemmArgs& a, const float* dy, const float* wd, float* dx, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                         int stride, int pad, int accumulate, int seg_n0 = 0, const lmkd_amax_desc* am = nullptr) {
  if (seg_n0 <= 0 || seg_n0 >= N) seg_n0 = 0;
  LMKD_REQUIRE(!seg_n0 || conv_planes(), "lmkd_conv2d_bwd_data_seg: two frame segments exist in the bf16-plane modes");
  LMKD_REQUIRE(Cout % 32 == 0, "lmkd_conv2d_bwd_data: Cout=%d must be a multiple of 32", Cout);
  LMKD_REQUIRE(stride == 1 || stride == 2, "lmkd_conv2d_bwd_data: stride %d unsupported", stride);
  LMKD_REQUIRE(KH * KW <= LMKD_MAX_TAPS, "lmkd_conv2d_bwd_data: kernel too large");
  LMKD_REQUIRE(!g_lmkd_act_bf16 || conv_nprod() == 1, "bf16 activations need lmkd_conv_set_compute_dtype(1)");
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  LMKD_REQUIRE((long)N * H * W * Cin < 2147483647L && (long)N * Ho * Wo * Cout < 2147483647L,
               "lmkd_conv2d_bwd_data: tensor exceeds 2^31 elements");
  LMKD_REQUIRE(!conv_planes() || (long)N * Ho * Wo * Cout * (g_lmkd_act_bf16 ? 2 : 4) < 0xffffffe0L,
               "lmkd_conv2d_bwd_data: dy exceeds the 4 GiB buffer range of the bf16-plane kernels");
  dgrad_geometry(a, N, H, W, Cin, Cout, KH, KW, stride, pad, seg_n0);
  a.src = dy; a.wpk = wd; a.out = dx; a.accum = accumulate;
  a.h2_xw = am ? (const unsigned*)am->dy_words : nullptr;
  return LMKD_OK;
}

extern "C" int lmkd_conv2d_bwd_data(const float* dy, const float* wd, float* dx, int N, int H, int W, int Cin, int Cout,
                                    int KH, int KW, int stride, int pad, int accumulate, void* stream) {
  LMKD_REQUIRE(dy && wd && dx, "lmkd_conv2d_bwd_data: null pointer");
  LMKD_REQUIRE(aligned16(dy) && aligned16(wd), "lmkd_conv2d_bwd_data: operands must be 16-byte aligned");
  ConvGemmArgs a;
  if (const int rc = bwd_data_args(a, dy, wd, dx, N, H, W, Cin, Cout, KH, KW, stride, pad, accumulate)) return rc;
  return launch_conv(a, plan_dgrad(a), (hipStream_t)stream);
}

// The data gradient that feeds relu + train-mode BatchNorm backward (BasicBlock: d a1 = dgrad(conv2), a1 = relu(bn1(c1));
// resnet18_2fc.py:41-42 runs torchvision's block): the epilogue of the patch kernel also reads the BatchNorm's input at the pixels it
// has just produced and leaves the per-row-tile sums (sum g, sum g * xhat) in `part`, so lmkd_bn_backward_part needs no reduction pass
// over (dx, bn_x).  Exists for the launches conv_patch16_x3_kernel serves (stride 1, three-plane arithmetic, fp32 tensors, 128-row
// tiles); lmkd_conv2d_bwd_data_bn_tiles returns the row count of `part` ([tiles][Cin][2] floats) or 0 when the launch has no such form.
extern "C" int lmkd_conv2d_bwd_data_bn_tiles_seg(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int seg_n0, int* tiles0) {
  if (stride != 1 || Cout % 32 != 0 || KH * KW > LMKD_MAX_TAPS) return 0;
  ConvGemmArgs a;
  if (bwd_data_args(a, nullptr, nullptr, nullptr, N, H, W, Cin, Cout, KH, KW, stride, pad, 0, seg_n0)) return 0;
  const ConvPlan p = plan_dgrad(a);
  if (!p.bnb_form) return 0;
  if (tiles0) *tiles0 = p.seg_t0;
  return p.tiles_per_class;
}
extern "C" int lmkd_conv2d_bwd_data_bn_tiles(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
  return lmkd_conv2d_bwd_data_bn_tiles_seg(N, H, W, Cin, Cout, KH, KW, stride, pad, 0, nullptr);
}
// lmkd_conv2d_bwd_data / lmkd_conv2d_bwd_data_bn (bn_x / bn_stats / part nullable together) over two frame segments (lmkd_conv2d_fwd_seg):
// bn_stats is a [2][5][Cin] table, part has lmkd_conv2d_bwd_data_bn_tiles_seg rows.  Bit-identical to two launches on the halves.
extern "C" int lmkd_conv2d_bwd_data_seg(const float* dy, const float* wd, float* dx, const float* bn_x, const float* bn_stats, float* part, int N,
                                        int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int accumulate, int seg_n0, void* stream,
                                        const lmkd_amax_desc* amax) {
  LMKD_REQUIRE(dy && wd && dx, "lmkd_conv2d_bwd_data_seg: null pointer");
  LMKD_REQUIRE(aligned16(dy) && aligned16(wd), "lmkd_conv2d_bwd_data_seg: operands must be 16-byte aligned");
  LMKD_REQUIRE((bn_x != nullptr) == (bn_stats != nullptr) && (bn_x != nullptr) == (part != nullptr), "lmkd_conv2d_bwd_data_seg: bn_x, bn_stats and part go together");
  ConvGemmArgs a;
  if (const int rc = bwd_data_args(a, dy, wd, dx, N, H, W, Cin, Cout, KH, KW, stride, pad, accumulate, seg_n0, amax)) return rc;
  note_fenced(amax);
  if (bn_x) {
    LMKD_REQUIRE(!accumulate && aligned16(bn_x) && aligned16(bn_stats), "lmkd_conv2d_bwd_data_seg: the fused BatchNorm sums need a plain (non-accumulating) launch and aligned operands");
    a.bnb_x = bn_x; a.bnb_stats = bn_stats; a.stat_partial = part;
  }
  const ConvPlan p = plan_dgrad(a);
  LMKD_REQUIRE(!bn_x || p.bnb_form, "lmkd_conv2d_bwd_data_seg: this launch has no fused form (lmkd_conv2d_bwd_data_bn_tiles_seg returned 0)");
  return launch_conv(a, p, (hipStream_t)stream);
}
extern "C" int lmkd_conv2d_bwd_data_bn(const float* dy, const float* wd, float* dx, const float* bn_x, const float* bn_stats, float* part,
                                       int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, void* stream) {
  LMKD_REQUIRE(dy && wd && dx && bn_x && bn_stats && part, "lmkd_conv2d_bwd_data_bn: null pointer");
  LMKD_REQUIRE(aligned16(dy) && aligned16(wd) && aligned16(bn_x) && aligned16(bn_stats), "lmkd_conv2d_bwd_data_bn: operands must be 16-byte aligned");
  ConvGemmArgs a;
  if (const int rc = bwd_data_args(a, dy, wd, dx, N, H, W, Cin, Cout, KH, KW, stride, pad, 0)) return rc;
  a.bnb_x = bn_x; a.bnb_stats = bn_stats; a.stat_partial = part;
  const ConvPlan p = plan_dgrad(a);
  LMKD_REQUIRE(p.bnb_form, "lmkd_conv2d_bwd_data_bn: this launch has no fused form (lmkd_conv2d_bwd_data_bn_tiles returned 0)");
  return launch_conv(a, p, (hipStream_t)stream);
}

// Split-K plan of the weight gradient.  Output tiles are few (Cout x 9*Cin is small) and the reduction is long, so the
// pixel range is split over gridDim.z.  The split count is chosen so that the launch is (just under) a whole number of
// rounds of resident workgroups: an arbitrary count leaves a 1.5-round launch that runs as long as a 2-round one.
static int g_wgrad_planes = 1;   // bf16 / 3xbf16 modes: weight gradient on the bf16-plane kernel (wgrad_x3.h); 0 = fp32-tile kernel
extern "C" int lmkd_conv_set_wgrad_planes(int on) { g_wgrad_planes = on ? 1 : 0; return LMKD_OK; }
// 3x3 / stride-1 weight gradients of the bf16-plane modes from a rolling LDS window of x (wgrad_win.h); 0 = im2col-gather kernel
static int g_wgrad_win16 = 1;      // three-plane modes, fp32 tensors: conv_wgrad_win16_kernel (v_mfma_f32_16x16x32_bf16); 0 = the 32x32x16 form
extern "C" int lmkd_conv_set_wgrad_win16(int on) { g_wgrad_win16 = on ? 1 : 0; return LMKD_OK; }
static int g_wgrad_window = 1;
extern "C" int lmkd_conv_set_wgrad_window(int on) { g_wgrad_window = on < 0 ? 0 : on; return LMKD_OK; }      // > 1: workgroup target of the split plan
static inline bool wgrad_win_eligible(int W, int Cs, int Cout, int KH, int KW, int stride, int pad) {
  return g_wgrad_window && g_wgrad_planes && conv_planes() && KH == 3 && KW == 3 && stride == 1 && pad == 1 &&
         Cs % 32 == 0 && 32 + 2 * (W + 1) <= 256;
}
// pixel splits: ONE round of resident workgroups (two per CU; four of the two-wave workgroups of the one-plane modes - registers
// allow two waves per SIMD, one for the three-plane Cout = 64 instance) - measured at 200 frames (tools/wgrad_bench.py): 277 / 228 /
// 225 / 229 us per layer against 348 / 273 / 244 / 246 with twice as many, shorter slabs (the window warm-up and the slab traffic
// double) - but no slab shorter than 12 steps per warm-up chunk of the window (rows [k0 - halo, k0 + halo) precede the first MFMA)
static void wgrad_win_plan(int Mpix, int W, int Cs, int Cout, int* cob, int* splits, int* steps_per_split) {
  *cob = Cout >= 128 ? 4 : 2;
  const int tiles = cdiv(Cout, 32 * *cob) * (Cs / 32);
  const int steps = cdiv(Mpix, LMKD_BK);
  const int warm = cdiv(2 * (W + 1), LMKD_BK);
  const int resident = 256 * ((conv_nprod() >= 6 && *cob == 2) ? 2 : 8 / *cob);
  // Round 5: the number of slabs is proportional to the segment's WORK, one round of resident workgroups for a whole 400-frame episode
  // (steps x tiles = 39 200 x 4 / cob on every 3x3 layer of the trunk), not one round per call: since round 4 the support and the query call are
  // ONE launch over two frame segments, each planned on its own (so that the merged and the two-call form stay bit-identical, the plan may
  // depend on nothing but the segment) - which made every merged launch 1 024 workgroups = two rounds of shorter slabs.  Per launch over
  // 200 + 200 frames, window kernel + slab reduce (tools/wgrad_split_ab.py, profiles/r05_wgrad_split_ab.txt): 386 / 286 / 275 / 268 us ->
  // 288 - 345 / 259 / 252 / 250.  At least 128 workgroups per segment (small episodes).
  int sp = g_wgrad_window > 1 ? cdiv(g_wgrad_window, tiles)
                              : std::max((int)(((long)resident * steps + 19600L * 4 / *cob) / (39200L * 4 / *cob)), cdiv(128, tiles));      // (to nearest)
  const int cap = std::max(1, steps / (12 * warm));
  if (sp > cap) sp = cap;
  *steps_per_split = cdiv(steps, sp);
  *splits = cdiv(steps, *steps_per_split);
}

static void wgrad_plan(int Mpix, int Cout, int Kp, int* splits, int* steps_per_split, int* bm, int* bn, bool planes = false) {
  // both operands are K-outer here (b32 fragment reads): the 128-wide tiles (1 read per MFMA) beat 64x64 (2 per MFMA):
  // measured 91.6 vs 74.8 TFLOP/s over the trunk's weight gradients
  *bm = Cout <= 64 ? 64 : 128;
  *bn = (Kp % 128 == 0 && Kp >= 1024) ? 128 : 64;
  int per_cu = (*bm == 128 && *bn == 128) ? 2 : ((*bm == 64 && *bn == 64) ? 4 : 3);
  if (planes) {      // wgrad_x3.h: 4-wave workgroups, LDS = planes x 32 k rows x (2 bytes per column + 64) per operand
    if (*bm == 64 && *bn == 128) *bn = 64;
    const int npl = conv_nprod() == 1 ? 1 : 3;
    const long lds = 1L * npl * LMKD_BK * ((*bm * 2 + 64) + (*bn * 2 + 64));      // single LDS buffer
    per_cu = (int)(160 * 1024 / lds);
    if (per_cu > 4) per_cu = 4;
    if (per_cu < 1) per_cu = 1;
  }
  const int tiles = cdiv(Cout, *bm) * cdiv(Kp, *bn);
  const int steps = cdiv(Mpix, LMKD_BK);
  const int slots = 256 * per_cu;
  int best_sp = 1;
  double best_cost = 1e30;
  for (int r = 1; r <= 3; ++r) {            // (just under) r whole rounds of resident workgroups
    int sp = (slots * r) / tiles;
    if (sp > steps / 4) sp = steps / 4;
    if (sp < 1) sp = 1;
    const int sps = cdiv(steps, sp);
    sp = cdiv(steps, sps);
    const double rounds = (double)cdiv((long)tiles * sp, slots);
    // cost: K-steps executed per slot, plus the slab write + reduce traffic expressed in K-step units
    const double cost = rounds * sps + 1.0 * sp / 8.0;
    if (cost < best_cost) { best_cost = cost; best_sp = sp; }
  }
  // Cout <= 64 (stem, layer 1: reductions over 0.6 - 2.5 M pixels) on the bf16-plane kernel: slabs of at most 64 K-steps.
  // A rounding error of the MFMA accumulation is then relative to a 2 K-pixel partial sum instead of a 10 K-pixel one and the
  // slabs are summed by the reduce kernel (blocked summation; measured against fp64 on the 200-frame stem: relative L2 error
  // 8.3e-6 -> 1.9e-6, the fp32 MFMA kernel's level).  The extra slabs are a few tens of MB per launch.
  if (planes && *bm == 64 && *bn == 64 && best_sp < cdiv(steps, 64)) best_sp = cdiv(steps, 64);
  *steps_per_split = cdiv(steps, best_sp);
  *splits = cdiv(steps, *steps_per_split);
}

// the stem's weight gradient on stem_wgrad_kernel (wgrad_stem.h): three-plane modes, fp32 tensors, 64 output channels, rows of 17 - 128
// output pixels.  -> slabs (0: not that kind of launch), units per slab
static int g_wgrad_stem = 1;
extern "C" int lmkd_conv_set_wgrad_stem(int on) { g_wgrad_stem = on ? 1 : 0; return LMKD_OK; }
static int stem_wgrad_plan(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, int* G) {
  if (!g_wgrad_stem || !g_wgrad_planes || conv_nprod(g_lmkd_act_bf16) < 6 || Cs != 4 || Cout != 64 || KH != 7 || KW != 7 || stride != 2 || pad != 3) return 0;
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  if (Wo < 17 || Wo > 128 || W > 2 * Wo || Ho < 1) return 0;      // >= 2 steps of 32 pixels per unit; LDS: 60 * (16 Wo + 64) + 30720 bytes
  const int units = N * cdiv(Ho, 2);
  int g = std::max(1, 2048 / (2 * Wo));                 // about 2048 pixels per slab (wgrad_plan: the accumulation error of a long partial sum)
  g = std::min(g, std::max(1, units / 256));            // but at least one slab per CU where the problem has that many units
  *G = g;
  return cdiv(units, g);
}

// ---- weight-gradient plan --------------------------------------------------------------------------
// Which kernel a weight gradient runs, with its pixel splits, grid and workspace: decided once, by plan_wgrad, for the launch
// (launch_wgrad), the report (lmkd_conv2d_plan kind 2) and the workspace size (lmkd_conv2d_bwd_weight_workspace_seg).
enum class WgFam : unsigned char {
  Stem,       // stem_wgrad_kernel (wgrad_stem.h), reported as id 14
  Win16,      // rolling window on the 16x16x32 MFMA (conv_wgrad_win16_kernel), ids 5 / 6 = 128 / 64 output channels per workgroup
  Win,        // rolling window on the 32x32x16 MFMA (conv_wgrad_win_kernel), ids 5 / 6
  Planes,     // bf16-plane im2col gather (conv_wgrad_x3_kernel), ids 1 - 4 by tile
  Tile,       // fp32 MFMA tiles (conv_wgrad_kernel), ids 1 - 4 by tile
};
struct WgradPlan {
  WgFam fam;
  bool pre, act16, smallc;
  int nprod;              // conv_nprod of the launch
  int bm, bn;             // Planes / Tile: output tile (Cout x packed K)
  int cob;                // Win16 / Win: 32-channel blocks of Cout per workgroup (COB)
  int G;                  // Stem: units per slab
  int splits, splits0, sps0, sps1, seg_pix0;      // pixel splits (all / of segment 0), K-steps per split of each segment, segment 0's pixels
  int xcd;                // Planes / Tile: all tiles of a pixel split on one XCD
  int grid;
  long need;              // workspace bytes the launch writes
  long ws;                // workspace bytes lmkd_conv2d_bwd_weight_workspace(_seg) reports
};

// workspace of one launch without frame segments: the larger of the gather and the window kernel's split plans
static long wgrad_workspace(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad) {
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  const int Kp = KH * kw_padded(Cs, KW) * Cs;
  int G, splits, sps, bm, bn;
  if (const int slabs = stem_wgrad_plan(N, H, W, Cs, Cout, KH, KW, stride, pad, &G)) return (long)slabs * Cout * Kp * sizeof(float);
  wgrad_plan(N * Ho * Wo, Cout, Kp, &splits, &sps, &bm, &bn, conv_planes() && g_wgrad_planes);
  if (wgrad_win_eligible(W, Cs, Cout, KH, KW, stride, pad)) {
    int cob, wsplits, wsps;
    wgrad_win_plan(N * Ho * Wo, W, Cs, Cout, &cob, &wsplits, &wsps);
    splits = std::max(splits, wsplits);
  }
  return (long)splits * Cout * Kp * sizeof(float);
}

// seg_n0: two frame segments [0, seg_n0) | [seg_n0, N) (0: one); pre: relu(BatchNorm(x)) in the loader; maxima: the caller named max |x|
// and max |dy|
static WgradPlan plan_wgrad(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, int seg_n0, bool pre, bool maxima) {
  WgradPlan p;
  memset(&p, 0, sizeof(p));
  const bool act16 = g_lmkd_act_bf16;
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  const int Kp = KH * kw_padded(Cs, KW) * Cs, Mpix = N * Ho * Wo;
  p.pre = pre; p.act16 = act16; p.smallc = Cs == 4;
  // each frame segment is split into the slabs a launch of its own would use - the same partial sums (a slab's length bounds the MFMA
  // accumulation error, wgrad_plan), twice the workgroups - so the workspace is the larger of the whole launch's and the two segments'
  // (the stem's kernel has no segments: its one-launch plan)
  p.ws = wgrad_workspace(N, H, W, Cs, Cout, KH, KW, stride, pad);
  if (seg_n0)
    p.ws = std::max(p.ws, wgrad_workspace(seg_n0, H, W, Cs, Cout, KH, KW, stride, pad) + wgrad_workspace(N - seg_n0, H, W, Cs, Cout, KH, KW, stride, pad));
  p.seg_pix0 = seg_n0 ? seg_n0 * Ho * Wo : Mpix;
  if (const int slabs = stem_wgrad_plan(N, H, W, Cs, Cout, KH, KW, stride, pad, &p.G)) {
    p.fam = WgFam::Stem;
    p.nprod = conv_nprod(false, maxima);
    // one workgroup per slab (the kernel can also walk several): a grid of exactly one resident workgroup per CU ran in TWO rounds
    // whenever a CU was not free (583 us alone, erratic beside other streams)
    p.splits = p.grid = slabs;
  } else if (wgrad_win_eligible(W, Cs, Cout, KH, KW, stride, pad)) {
    const bool w16 = g_wgrad_win16 && conv_nprod(act16) >= 6;      // three-plane modes, fp32 tensors: the 16x16x32 MFMA form
    p.fam = w16 ? WgFam::Win16 : WgFam::Win;
    p.nprod = w16 ? conv_nprod(false, maxima) : conv_nprod(act16);
    wgrad_win_plan(Mpix, W, Cs, Cout, &p.cob, &p.splits, &p.sps0);
    p.splits0 = p.splits;
    if (seg_n0) {
      int sp1, cob1;
      wgrad_win_plan(p.seg_pix0, W, Cs, Cout, &p.cob, &p.splits0, &p.sps0);
      wgrad_win_plan(Mpix - p.seg_pix0, W, Cs, Cout, &cob1, &sp1, &p.sps1);
      p.splits = p.splits0 + sp1;
    }
    p.grid = 8 * cdiv(p.splits, 8) * cdiv(Cout, 32 * p.cob) * (Cs / 32);
  } else {
    const bool planes = conv_planes() && g_wgrad_planes;
    p.fam = planes ? WgFam::Planes : WgFam::Tile;
    // conv_wgrad_x3_kernel's two-plane form: not the padded stem input, not the BatchNorm loader
    p.nprod = planes ? conv_nprod(act16, maxima && !p.smallc && !pre) : (conv_nprod() == 1 ? 1 : 0);      // (Tile: bf16 inputs in mode 1)
    wgrad_plan(Mpix, Cout, Kp, &p.splits, &p.sps0, &p.bm, &p.bn, planes);
    p.splits0 = p.splits;
    if (seg_n0) {
      int sp1, bm1, bn1;
      wgrad_plan(p.seg_pix0, Cout, Kp, &p.splits0, &p.sps0, &p.bm, &p.bn, planes);
      wgrad_plan(Mpix - p.seg_pix0, Cout, Kp, &sp1, &p.sps1, &bm1, &bn1, planes);      // (the tile shape depends on Cout and Kp only)
      p.splits = p.splits0 + sp1;
    }
    // all column tiles of one pixel split read the same x / dy rows: with >= 32 splits they are dealt to ONE XCD (ids congruent
    // mod 8), whose L2 then serves the re-reads.  PMC: FETCH_SIZE 1053 -> 279 MB per launch (algorithmic 160-320 MB); the kernel
    // alone is a few % slower on layer 1, the two-stream episode is unchanged (20.5 episodes/s), so it is on by default;
    // lmkd_conv_set_xcd_mode(1) keeps the plain order
    p.xcd = (g_xcd_mode != 0 && g_xcd_mode != 1 && p.splits >= 32) ? 1 : 0;
    p.grid = (p.xcd ? 8 * cdiv(p.splits, 8) : p.splits) * cdiv(Cout, p.bm) * cdiv(Kp, p.bn);
  }
  p.need = (long)p.splits * Cout * Kp * sizeof(float);
  return p;
}

// stem_wgrad_kernel
template <int NPROD, int D, int RLC>
static void launch_stem_wgrad(const StemWgradArgs& w, dim3 grid, size_t lds, hipStream_t s) {
  lds_attr_once<stem_wgrad_kernel<NPROD, D, RLC>>(160 * 1024);
  hipLaunchKernelGGL((stem_wgrad_kernel<NPROD, D, RLC>), grid, dim3(512), lds, s, w);
}
template <int NPROD>
static void launch_stem_wgrad(const StemWgradArgs& w, dim3 grid, size_t lds, hipStream_t s) {
  const bool deep = cdiv(2 * w.Wo, 32) >= 6;      // dy tiles fetched six steps ahead (224-pixel images: seven steps per unit), else two
  if (deep && w.RL == 1856) launch_stem_wgrad<NPROD, 6, 1856>(w, grid, lds, s);      // 224-pixel images
  else if (deep) launch_stem_wgrad<NPROD, 6, 0>(w, grid, lds, s);
  else launch_stem_wgrad<NPROD, 2, 0>(w, grid, lds, s);
}
// conv_wgrad_win16_kernel / conv_wgrad_win_kernel with COB channel blocks
template <int COB>
static void launch_wgrad_win(const WgradWinArgs& w, const WgradPlan& p, bool big, hipStream_t s) {
  const dim3 grid(p.grid);
  if (p.fam == WgFam::Win16) {
    // Cout = 64 (two channel blocks): the second pair of waves takes the other 16 input channels of all nine taps
    constexpr int JW = COB == 2 ? 1 : 2;
    constexpr int NT = 64 * COB * (2 / JW);
    with_nprod<3, 6, 9>(p.nprod, [&](auto np) {
      if (big && p.pre) hipLaunchKernelGGL((conv_wgrad_win16_kernel<COB, np, 256, true, 9, JW>), grid, dim3(NT), 0, s, w);
      else if (big) hipLaunchKernelGGL((conv_wgrad_win16_kernel<COB, np, 256, false, 9, JW>), grid, dim3(NT), 0, s, w);
      else if (p.pre) hipLaunchKernelGGL((conv_wgrad_win16_kernel<COB, np, 128, true, 9, JW>), grid, dim3(NT), 0, s, w);
      else hipLaunchKernelGGL((conv_wgrad_win16_kernel<COB, np, 128, false, 9, JW>), grid, dim3(NT), 0, s, w);
    });
    return;
  }
  auto go = [&](auto np, auto a16, auto pre) {
    constexpr int NPROD = decltype(np)::value;
    constexpr bool A16 = decltype(a16)::value, PRE = decltype(pre)::value;
    // Cout = 64 leaves two channel blocks: in the three-plane modes the nine taps are dealt 5 + 4 to two wave groups (four waves
    // instead of two: 262 vs 318 us at 200 frames); with one plane the extra dy-fragment reads cost more (119 vs 94)
    constexpr int TPW = (COB == 2 && NPROD != 1) ? 5 : 9;
    constexpr int NT = 64 * COB * ((9 + TPW - 1) / TPW);
    if (big) hipLaunchKernelGGL((conv_wgrad_win_kernel<COB, NPROD, A16, 256, PRE, TPW>), grid, dim3(NT), 0, s, w);
    else hipLaunchKernelGGL((conv_wgrad_win_kernel<COB, NPROD, A16, 128, PRE, TPW>), grid, dim3(NT), 0, s, w);
  };
  using T = std::true_type;
  using F = std::false_type;
  if (p.act16) go(std::integral_constant<int, 1>{}, T{}, F{});
  else with_nprod<1, 6, 9>(p.nprod, [&](auto np) { if (p.pre) go(np, F{}, T{}); else go(np, F{}, F{}); });
}

// conv_wgrad_x3_kernel
template <class CFG>
static void launch_wgrad_planes(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  const dim3 grid(p.grid), block(256);
  if (p.act16) {
    if (p.smallc) hipLaunchKernelGGL((conv_wgrad_x3_kernel<CFG, true, 1, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_wgrad_x3_kernel<CFG, false, 1, false, true>), grid, block, 0, s, a);
  } else if (p.smallc) {
    with_nprod<1, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_wgrad_x3_kernel<CFG, true, np, false>), grid, block, 0, s, a); });
  } else if (p.pre) {
    with_nprod<1, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_wgrad_x3_kernel<CFG, false, np, true>), grid, block, 0, s, a); });
  } else {
    with_nprod<1, 3, 6, 9>(p.nprod, [&](auto np) { hipLaunchKernelGGL((conv_wgrad_x3_kernel<CFG, false, np, false>), grid, block, 0, s, a); });
  }
}

// conv_wgrad_kernel
template <class CFG, bool SM, int THR>
static void launch_wgrad_tile(const WgradArgs& a, const WgradPlan& p, hipStream_t s) {
  const dim3 grid(p.grid);
  if (p.nprod == 1) hipLaunchKernelGGL((conv_wgrad_kernel<CFG, SM, true>), grid, dim3(THR), 0, s, a);
  else if (!SM && p.pre) hipLaunchKernelGGL((conv_wgrad_kernel<CFG, false, false, true>), grid, dim3(THR), 0, s, a);
  else hipLaunchKernelGGL((conv_wgrad_kernel<CFG, SM, false>), grid, dim3(THR), 0, s, a);
}

// dw_oihw[Cout,Cin,KH,KW] from x[N,H,W,Cs] (Cs >= Cin channel-padded) and dy[N,Ho,Wo,Cout]
static int conv2d_bwd_weight_impl(const float* x, const float* pre_stats, const float* dy, float* dw_oihw, float* workspace,
                                  long ws_bytes, int N, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                  void* stream, int accumulate = 0, int seg_n0 = 0, const lmkd_amax_desc* am = nullptr) {
  const unsigned* amax_x = am ? (const unsigned*)am->x_words : nullptr;
  const unsigned* amax_dy = am ? (const unsigned*)am->dy_words : nullptr;
  note_fenced(am);
  LMKD_REQUIRE(x && dy && dw_oihw && workspace, "lmkd_conv2d_bwd_weight: null pointer");
  // two frame segments: each is split into the slabs a launch of its own would use (same partial sums, same accumulation error), the
  // PRE loader takes the segment's BatchNorm table, ONE slab reduce sums everything
  if (seg_n0 <= 0 || seg_n0 >= N) seg_n0 = 0;
  LMKD_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(workspace), "lmkd_conv2d_bwd_weight: operands must be 16-byte aligned");
  LMKD_REQUIRE(Cs % 32 == 0 || Cs == 4, "lmkd_conv2d_bwd_weight: channel count %d must be 4 or a multiple of 32", Cs);
  LMKD_REQUIRE(Cout % 4 == 0, "lmkd_conv2d_bwd_weight: Cout %% 4 != 0");
  const bool smallc = Cs == 4;
  const WgradPlan p = plan_wgrad(N, H, W, Cs, Cout, KH, KW, stride, pad, seg_n0, pre_stats != nullptr, amax_x && amax_dy);
  LMKD_REQUIRE(!seg_n0 || p.fam != WgFam::Tile, "lmkd_conv2d_bwd_weight_seg: two frame segments exist in the bf16-plane modes");
  LMKD_REQUIRE(!pre_stats || (!smallc && (conv_nprod() != 1 || p.fam != WgFam::Tile) && !p.act16), "lmkd_conv2d_bwd_weight_pre: Cs %% 32 == 0, fp32 activations only");
  LMKD_REQUIRE(!p.act16 || (conv_nprod() == 1 && p.fam != WgFam::Tile), "bf16 activations need lmkd_conv_set_compute_dtype(1) and the plane weight-gradient kernel");
  const int Ho = conv_out(H, KH, stride, pad), Wo = conv_out(W, KW, stride, pad);
  const int KWp = kw_padded(Cs, KW), Kp = KH * KWp * Cs, Mpix = N * Ho * Wo;
  LMKD_REQUIRE((long)N * H * W * Cs < 2147483647L && (long)Mpix * Cout < 2147483647L, "lmkd_conv2d_bwd_weight: tensor too large");
  LMKD_REQUIRE(ws_bytes >= p.need, "lmkd_conv2d_bwd_weight: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  if (p.fam == WgFam::Stem) {
    LMKD_REQUIRE((long)Mpix * 64 * 4 < 0xffffffe0L && (long)N * H * W * 16 < 0xffffffe0L, "lmkd_conv2d_bwd_weight: tensor too large for 32-bit byte offsets");
    StemWgradArgs w;
    memset(&w, 0, sizeof(w));
    w.dy = dy; w.x = x; w.slab = workspace;
    w.h2_xw = amax_x; w.h2_dyw = amax_dy;
    w.N = N; w.H = H; w.W = W; w.Ho = Ho; w.Wo = Wo;
    w.upi = cdiv(Ho, 2); w.units = N * w.upi; w.G = p.G; w.slabs = p.splits;
    w.RL = 16 * Wo + 64;
    const size_t lds = (size_t)2 * 10 * 3 * w.RL + 2 * 3 * STEM_WG_APLANE;
    with_nprod<3, 6, 9>(p.nprod, [&](auto np) { launch_stem_wgrad<np>(w, dim3(p.grid), lds, s); });
    LMKD_CHECK_LAUNCH("stem_wgrad_kernel");
    if (Kp <= 256) {
      hipLaunchKernelGGL(wgrad_reduce_stem_kernel, dim3(Cout), dim3(256, 4), 0, s, (const float*)workspace, dw_oihw, p.splits, Cout, Cin, Cs, KH, KW,
                         KWp, Kp, accumulate);
    } else {
      launch_wgrad_reduce((const float*)workspace, dw_oihw, p.splits, Cout, Cin, Cs, KH, KW, KWp, Kp, accumulate, s);
    }
    LMKD_CHECK_LAUNCH("wgrad_reduce_kernel");
    return LMKD_OK;
  }
  if (p.fam == WgFam::Win16 || p.fam == WgFam::Win) {
    LMKD_REQUIRE((long)Mpix * std::max(Cs, Cout) * 4 < 2147483647L, "lmkd_conv2d_bwd_weight: tensor too large for 32-bit byte offsets");
    WgradWinArgs w;
    memset(&w, 0, sizeof(w));
    w.dy = dy; w.x = x; w.slab = workspace; w.pre_stats = pre_stats;
    w.h2_xw = amax_x; w.h2_dyw = amax_dy;
    w.N = N; w.H = H; w.W = W; w.Cs = Cs; w.Co = Cout; w.Kp = Kp; w.Mpix = Mpix;
    w.steps_total = cdiv(Mpix, LMKD_BK);
    w.splits = p.splits; w.steps_per_split = p.sps0;
    w.seg_pix0 = p.seg_pix0; w.seg_splits0 = p.splits0; w.sps1 = p.sps1;
    w.n_ct = cdiv(Cout, 32 * p.cob); w.n_it = Cs / 32;
    w.div_hw = make_fastdiv(H * W); w.div_w = make_fastdiv(W);
    const bool big = 32 + 2 * (W + 1) > 128;      // ring of 256 pixel rows instead of 128
    if (p.cob == 4) launch_wgrad_win<4>(w, p, big, s);
    else launch_wgrad_win<2>(w, p, big, s);
    LMKD_CHECK_LAUNCH("conv_wgrad_win_kernel");
    launch_wgrad_reduce((const float*)workspace, dw_oihw, p.splits, Cout, Cin, Cs, KH, KW, KWp, Kp, accumulate, s);
    LMKD_CHECK_LAUNCH("wgrad_reduce_kernel");
    return LMKD_OK;
  }
  WgradArgs a;
  memset(&a, 0, sizeof(a));
  a.dy = dy; a.x = x; a.slab = workspace; a.pre_stats = pre_stats;
  a.h2_xw = amax_x; a.h2_dyw = amax_dy;
  a.N = N; a.Hs = H; a.Ws = W; a.Cs = Cs;
  a.Ho = Ho; a.Wo = Wo; a.Co = Cout;
  a.stride = stride; a.pad = pad; a.KH = KH; a.KW = KW; a.KWp = KWp;
  a.Kp = Kp; a.Mpix = Mpix;
  a.steps_per_split = p.sps0;
  a.seg_pix0 = p.seg_pix0; a.seg_splits0 = p.splits0; a.sps1 = p.sps1;
  a.steps_total = cdiv(Mpix, LMKD_BK);
  a.div_hw = make_fastdiv(Ho * Wo); a.div_w = make_fastdiv(Wo);
  a.n_mt = cdiv(Cout, p.bm); a.n_jt = cdiv(Kp, p.bn); a.splits = p.splits;
  a.xcd_mode = p.xcd;
  const int bm = p.bm, bn = p.bn;
  LMKD_REQUIRE(!smallc || (bm == 64 && bn == 64), "lmkd_conv2d_bwd_weight: padded-stem path expects Cout <= 64");
  if (p.fam == WgFam::Planes) {
    if (bm == 128 && bn == 128) launch_wgrad_planes<WgCfg<128, 128, 2, 2>>(a, p, s);
    else if (bm == 128) launch_wgrad_planes<WgCfg<128, 64, 2, 2>>(a, p, s);
    else launch_wgrad_planes<WgCfg<64, 64, 2, 2>>(a, p, s);
    LMKD_CHECK_LAUNCH("conv_wgrad_x3_kernel");
  } else {
    if (smallc) launch_wgrad_tile<TileCfg<64, 64, 2, 2>, true, LMKD_THREADS>(a, p, s);
    else if (bm == 64 && bn == 64) launch_wgrad_tile<TileCfg<64, 64, 2, 2>, false, LMKD_THREADS>(a, p, s);
    else if (bm == 128 && bn == 64) launch_wgrad_tile<TileCfg<128, 64, 2, 2>, false, LMKD_THREADS>(a, p, s);
    else if (bm == 64 && bn == 128) launch_wgrad_tile<TileCfg<64, 128, 2, 2>, false, LMKD_THREADS>(a, p, s);
    else launch_wgrad_tile<TileCfg<128, 128, 2, 4>, false, 512>(a, p, s);      // 8 waves: 4 per SIMD at 2 workgroups per CU
    LMKD_CHECK_LAUNCH("conv_wgrad_kernel");
  }
  launch_wgrad_reduce((const float*)workspace, dw_oihw, p.splits, Cout, Cin, Cs, KH, KW, KWp, Kp, accumulate, s);      // (stride-2 3x3 and 1x1 layers)
  LMKD_CHECK_LAUNCH("wgrad_reduce_kernel");
  return LMKD_OK;
}

// workspace of lmkd_conv2d_bwd_weight (and of the two-segment form, lmkd_conv2d_bwd_weight_seg: plan_wgrad)
extern "C" long lmkd_conv2d_bwd_weight_workspace_seg(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad, int seg_n0) {
  if (seg_n0 <= 0 || seg_n0 >= N) seg_n0 = 0;
  return plan_wgrad(N, H, W, Cs, Cout, KH, KW, stride, pad, seg_n0, false, false).ws;
}
extern "C" long lmkd_conv2d_bwd_weight_workspace(int N, int H, int W, int Cs, int Cout, int KH, int KW, int stride, int pad) {
  return lmkd_conv2d_bwd_weight_workspace_seg(N, H, W, Cs, Cout, KH, KW, stride, pad, 0);
}

extern "C" int lmkd_conv2d_bwd_weight(const float* x, const float* dy, float* dw_oihw, float* workspace, long ws_bytes,
                                      int N, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                      void* stream) {
  return conv2d_bwd_weight_impl(x, nullptr, dy, dw_oihw, workspace, ws_bytes, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad, stream);
}

// weight gradient of a convolution whose input was relu(BatchNorm(x_raw)) computed in the forward loader (lmkd_conv2d_fwd_pre):
// the same transform is applied to x_raw here, so the normalised activation is never stored
extern "C" int lmkd_conv2d_bwd_weight_pre(const float* x_raw, const float* pre_stats, const float* dy, float* dw_oihw,
                                          float* workspace, long ws_bytes, int N, int H, int W, int Cs, int Cin, int Cout, int KH,
                                          int KW, int stride, int pad, void* stream) {
  LMKD_REQUIRE(pre_stats, "lmkd_conv2d_bwd_weight_pre: BatchNorm table of the input missing");
  return conv2d_bwd_weight_impl(x_raw, pre_stats, dy, dw_oihw, workspace, ws_bytes, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad, stream);
}

// dw_oihw += weight gradient (dw_oihw is the parameter's .grad: gradient accumulation over the two trunk calls of an episode and
// over the episodes between two optimizer steps, trainwandb.py:141-143, without a separate add pass); pre_stats nullable
extern "C" int lmkd_conv2d_bwd_weight_acc(const float* x, const float* pre_stats, const float* dy, float* dw_oihw, float* workspace,
                                          long ws_bytes, int N, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int stride,
                                          int pad, void* stream) {
  return conv2d_bwd_weight_impl(x, pre_stats, dy, dw_oihw, workspace, ws_bytes, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad, stream, 1);
}


// weight gradient over two frame segments [0, seg_n0) | [seg_n0, N) of one tensor (lmkd_conv2d_fwd_seg): ONE launch + ONE slab reduce for
// both trunk calls of an episode; pre_stats (nullable) = [2][5][Cs] table; accumulate: dw_oihw += ; workspace:
// lmkd_conv2d_bwd_weight_workspace_seg bytes.  The split-K slabs are those of two separate launches; they are summed in one pass.
extern "C" int lmkd_conv2d_bwd_weight_seg(const float* x, const float* pre_stats, const float* dy, float* dw_oihw, float* workspace, long ws_bytes,
                                          int N, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int stride, int pad, int accumulate,
                                          int seg_n0, void* stream, const lmkd_amax_desc* amax) {
  return conv2d_bwd_weight_impl(x, pre_stats, dy, dw_oihw, workspace, ws_bytes, N, H, W, Cs, Cin, Cout, KH, KW, stride, pad, stream, accumulate, seg_n0, amax);
}

// Launch plan of a convolution, without launching: which kernel instance and tile order the three entry points above would
// pick for these shapes in the current arithmetic mode (info: 5 ints).  info[0] = tile id (lmkd_conv_set_tile numbering; the weight gradient
// reports 1 = 128x128/8 waves, 2 = 128x64, 3 = 64x64, 4 = 64x128), info[1] = XCD tile order (forward / data gradient: 0 row
// bands, 1 column slices; weight gradient: 1 = all tiles of a pixel split on one XCD), info[2] = pixel splits (weight gradient)
// or parity classes (data gradient), info[3] = workgroups launched.  Used by the parity tests to prove that the benchmark's
// kernel instances are the ones under test.  info[4] = 1 when the launch runs on the LDS-patch kernel (conv_patch.h) or, for the
// weight gradient, on the rolling-window kernel (wgrad_win.h; it reports tile id 5 = 128 output channels per workgroup, 6 = 64);
// info[4] = 2: the stem's kernels, tile id 14 - the input-row patch kernel (conv_stem.h; info[2] = 1) and the weight gradient's
// stem_wgrad_kernel (wgrad_stem.h; info[2] = slabs).
extern "C" int lmkd_conv2d_plan(int kind, int N, int H, int W, int Cs, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                int* info) {
  LMKD_REQUIRE(info && kind >= 0 && kind <= 2, "lmkd_conv2d_plan: kind must be 0 (forward), 1 (data gradient) or 2 (weight gradient)");
  LMKD_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0, "lmkd_conv2d_plan: bad shape");
  if (kind == 2) {
    const WgradPlan p = plan_wgrad(N, H, W, Cs, Cout, KH, KW, stride, pad, 0, false, false);
    info[1] = p.xcd; info[2] = p.splits; info[3] = p.grid;
    switch (p.fam) {
      case WgFam::Stem: info[0] = 14; info[4] = 2; break;
      case WgFam::Win16:
      case WgFam::Win: info[0] = p.cob == 4 ? 5 : 6; info[1] = 1; info[4] = 1; break;
      default: info[0] = (p.bm == 128 && p.bn == 128) ? 1 : (p.bm == 128 ? 2 : (p.bn == 128 ? 4 : 3)); info[4] = 0; break;
    }
    return LMKD_OK;
  }
  ConvGemmArgs a;
  if (kind == 0) fwd_geometry(a, N, H, W, Cs, Cout, KH, KW, stride, pad, 0);
  else dgrad_geometry(a, N, H, W, Cin, Cout, KH, KW, stride, pad, 0);
  const ConvPlan p = kind == 0 ? plan_fwd(a, KH, KW, pad) : plan_dgrad(a);
  info[0] = p.tile; info[1] = p.xcd; info[2] = p.nclass; info[3] = p.grid;
  info[4] = p.fam == ConvFam::Stem ? 2 : (p.fam == ConvFam::Patch || p.fam == ConvFam::Patch16 || p.fam == ConvFam::Patch1p ? 1 : 0);
  return LMKD_OK;
}
