// PNG decoding: the frames of depth / flow / RGB trees that the reference's teacher-side readers open with
// PIL.Image.open(path).convert("RGB") (teacher/code/AuxDataset.py:129-136, teacher/code/video_reader.py:190-199), decoded on the GPU
// bit for bit.  The shape is that of csrc/jpeg.hip:
//
//   lmkd_png_plan          host: walks the chunks of every image of a batch, checks the CRC-32 of IHDR / PLTE / IDAT / IEND and the zlib
//                          header, moves the IDAT payloads of a supported image together in place (one contiguous deflate stream per
//                          image), writes one descriptor per image and the palettes into a pool, and says per image: decoded here,
//                          unsupported (the caller decodes it with PIL) or malformed
//   lmkd_png_decode        two launches on the caller's stream:
//                            1. inflate, one wave per image: the wave copies the next window of compressed bytes into LDS, builds the
//                               block's code tables in LDS and decodes symbols one at a time (a serial job: every lane carries the
//                               same decoder state, so it lives in scalar registers and runs on the scalar unit; lane 0 stores);
//                               literals go into a 32 KiB LDS ring (the deflate window), a match or a piece of a stored block is
//                               copied by the whole wave, and the wave writes the ring out to the image's scanline scratch with
//                               coalesced stores
//                            2. unfilter + expand, one wave per image, rows in order: None / Up lane-parallel, Sub as a per-channel
//                               prefix sum, Average / Paeth serial along the row with one lane per byte of the pixel; the row is then
//                               written as RGB; the Adler-32 of the scanlines is folded row by row and compared with the trailer
//   lmkd_png_decode_host   the same routines (png_core.h) on the CPU (the tests' reference; not on the training path)
//
// Bounds, whatever the bytes say: compressed bytes are read through a window that clamps to the stream range; ring indices are masked;
// the bytes produced never exceed H * (stride + 1), which bounds every scratch write; a distance is checked against the bytes produced;
// each round of the decode loop consumes input or produces output; an error stops its own image only (status word).
#include "common.h"
#include "png_core.h"
#include <vector>

namespace {
using namespace pngcore;

struct PngDesc {
  long long sb, se;                       // deflate stream [sb, se) of the packed input (after the zlib header; the Adler-32 trailer inside)
  long long out_off;                      // byte offset of the image's uint8 [H][W][3] in the output
  long long scr_off;                      // byte offset of its H * (stride + 1) filtered scanline bytes in the scratch (16-byte aligned)
  int kind;                               // 0 = decoded by lmkd_png_decode, 1 = not
  int W, H;
  int ctype, bpp, stride;                 // colour type 0 / 2 / 3 / 6, bytes per pixel, bytes per row without the filter byte
  int pal_off;                            // byte offset of the 256 x 3 palette in the pool (type 3)
  int pad_;
};
static_assert(sizeof(PngDesc) % 8 == 0, "descriptor array");

// a lane of the wave in pngcore::inflate_windowed: its own iteration of every lane loop, the workgroup barrier between the phases
struct WaveDev {
  enum { STEP = 64, HELD = 1 };
  static __device__ __forceinline__ int first() { return (int)threadIdx.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ data, const PngDesc* __restrict__ descs,
                                                         uint8_t* __restrict__ scratch, int* __restrict__ status,
                                                         unsigned* __restrict__ trailer) {
  __shared__ __align__(16) uint8_t ring[RING];
  __shared__ __align__(16) uint8_t win[PWIN];
  __shared__ Huff lit, dst;
  __shared__ uint8_t lens[320];
  const PngDesc d = descs[blockIdx.x];
  int err = PE_OK;
  unsigned adler = 0;
  if (d.kind == 0)
    inflate_windowed<WaveDev>(data, d.sb, d.se, (long long)d.H * (d.stride + 1), scratch + d.scr_off, ring, win, lit, dst, lens, err, adler);
  if (threadIdx.x == 0) {
    status[blockIdx.x] = err;
    trailer[blockIdx.x] = adler;
  }
}

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// rowcap: bytes of one LDS row (>= the largest stride + 1 of the batch, a multiple of 16); dynamic LDS = 3 rows
__global__ __launch_bounds__(64) void png_unfilter_kernel(const PngDesc* __restrict__ descs, const uint8_t* __restrict__ pool,
                                                          const uint8_t* __restrict__ scratch, uint8_t* __restrict__ out,
                                                          int* __restrict__ status, const unsigned* __restrict__ trailer, int rowcap) {
  extern __shared__ __align__(16) uint8_t sm[];
  __shared__ unsigned psum[64][4];
  const int t = threadIdx.x;
  const PngDesc d = descs[blockIdx.x];
  if (d.kind != 0 || status[blockIdx.x] != 0) return;
  const int stride = d.stride, bpp = d.bpp, W = d.W, n = stride + 1;
  if (n > rowcap || bpp < 1 || bpp > 4 || (long long)W * bpp != stride) {      // (a descriptor the plan never writes)
    if (t == 0) status[blockIdx.x] = PE_WINDOW;
    return;
  }
  uint8_t* raw = sm;
  uint8_t* prev = sm + rowcap;
  uint8_t* cur = sm + 2 * rowcap;
  for (int i = t; i < stride; i += 64) prev[i] = 0;
  const uint8_t* pal = pool + (d.ctype == 3 ? d.pal_off : 0);
  uint8_t* o = out + d.out_off;
  unsigned A = 1, B = 0;
  int err = PE_OK;
  const int C = (W + 63) / 64;            // pixels per lane of the Sub prefix sum
  __syncthreads();
  for (int y = 0; y < d.H; ++y) {
    const uint8_t* g = scratch + d.scr_off + (long long)y * n;
    unsigned s1 = 0, s2 = 0;              // per lane at most 257 bytes: s2 <= 257 x 16385 x 255 < 2^31
    for (int i = t; i < n; i += 64) {
      const unsigned v = g[i];
      raw[i] = (uint8_t)v;
      s1 += v;
      s2 += (unsigned)(n - i) * v;
    }
    s1 = wave_sum_u(s1 % ADLER_MOD);
    s2 = wave_sum_u(s2 % ADLER_MOD);
    adler_combine(A, B, (unsigned)n, s1 % ADLER_MOD, s2 % ADLER_MOD);
    __syncthreads();
    const int ft = raw[0];
    if (ft > 4) {
      err = PE_FILTER;
      break;
    }
    const uint8_t* r = raw + 1;
    if (ft == 0) {
      for (int i = t; i < stride; i += 64) cur[i] = r[i];
    } else if (ft == 2) {
      for (int i = t; i < stride; i += 64) cur[i] = (uint8_t)(r[i] + prev[i]);
    } else if (ft == 1) {
      const int x0 = t * C < W ? t * C : W, x1 = x0 + C < W ? x0 + C : W;
      unsigned s[4] = {0, 0, 0, 0};
      for (int x = x0; x < x1; ++x)
        for (int k = 0; k < bpp; ++k) s[k] += r[x * bpp + k];
      for (int k = 0; k < 4; ++k) psum[t][k] = s[k];
      __syncthreads();
      unsigned c[4] = {0, 0, 0, 0};
      for (int j = 0; j < t; ++j)
        for (int k = 0; k < 4; ++k) c[k] += psum[j][k];
      for (int x = x0; x < x1; ++x)
        for (int k = 0; k < bpp; ++k) {
          c[k] = (c[k] + r[x * bpp + k]) & 255u;
          cur[x * bpp + k] = (uint8_t)c[k];
        }
    } else {
      if (t < bpp) unfilter_lane(ft, r, prev, cur, t, bpp, stride);
    }
    __syncthreads();
    for (int x = t; x < W; x += 64) expand_pixel(d.ctype, cur + x * bpp, pal, o + ((long long)y * W + x) * 3);
    uint8_t* tmp = prev;
    prev = cur;
    cur = tmp;
    __syncthreads();
  }
  if (t == 0) status[blockIdx.x] = err ? err : (((B << 16) | A) != trailer[blockIdx.x] ? PE_ADLER : PE_OK);
}

inline long long align16ll(long long v) { return (v + 15) & ~15LL; }

}  // namespace

extern "C" long lmkd_png_desc_bytes(void) { return (long)sizeof(PngDesc); }

extern "C" long lmkd_png_pool_bytes(int n) { return (long)(n > 0 ? n : 1) * 768; }

extern "C" const char* lmkd_png_reason(int reason) { return reason_text(reason); }

extern "C" int lmkd_png_plan(unsigned char* data, const long long* offsets, int n, void* descs, void* pool, long pool_cap, long long* info,
                             long long* totals) {
  LMKD_REQUIRE(n >= 0 && n <= 65535, "lmkd_png_plan: 0 <= n <= 65535 images per batch (got %d)", n);
  LMKD_REQUIRE(totals && (n == 0 || (data && offsets && descs && pool && info)), "lmkd_png_plan: null pointer");
  for (int i = 0; i < n; ++i)
    LMKD_REQUIRE(offsets[i] >= 0 && offsets[i + 1] >= offsets[i], "lmkd_png_plan: offsets must be non-decreasing (image %d)", i);
  PngDesc* D = (PngDesc*)descs;
  long used = 0;
  long long scr = 0, out_bytes = 0, supported = 0, max_stride = 0;
  std::vector<Parsed> holder(1);
  Parsed& P = holder[0];
  for (int i = 0; i < n; ++i) {
    const long long b = offsets[i], e = offsets[i + 1];
    P = Parsed();
    int reason = PR_NONE;
    const int verdict = parse_png(data + b, e - b, P, reason);
    PngDesc& d = D[i];
    memset(&d, 0, sizeof d);
    d.kind = 1;
    info[5 * i + 0] = verdict;
    info[5 * i + 1] = reason;
    info[5 * i + 2] = verdict == PST_MALFORMED ? 0 : P.H;
    info[5 * i + 3] = verdict == PST_MALFORMED ? 0 : P.W;
    info[5 * i + 4] = out_bytes;
    if (verdict == PST_MALFORMED) continue;
    d.out_off = out_bytes;
    out_bytes += (long long)P.H * P.W * 3;
    if (verdict != PST_OK) continue;
    d.kind = 0;
    d.W = P.W;
    d.H = P.H;
    d.ctype = P.ctype;
    d.bpp = P.bpp;
    d.stride = P.stride;
    d.sb = b + P.stream_begin;
    d.se = b + P.stream_end;
    d.scr_off = scr;
    scr += align16ll((long long)P.H * (P.stride + 1));
    if (P.ctype == 3) {
      LMKD_REQUIRE(used + 768 <= pool_cap, "lmkd_png_plan: palette pool of %ld bytes too small (lmkd_png_pool_bytes)", pool_cap);
      memcpy((unsigned char*)pool + used, P.pal, 768);
      d.pal_off = (int)used;
      used += 768;
    }
    ++supported;
    if (P.stride > max_stride) max_stride = P.stride;
  }
  totals[0] = used;
  totals[1] = scr;
  totals[2] = out_bytes;
  totals[3] = supported;
  totals[4] = max_stride;
  return LMKD_OK;
}

extern "C" int lmkd_png_decode(const unsigned char* data, const void* descs, const void* pool, int n, unsigned char* scratch,
                               unsigned char* out, int* status, unsigned* trailer, long long max_stride, void* stream) {
  LMKD_REQUIRE(n >= 0 && n <= 65535, "lmkd_png_decode: 0 <= n <= 65535 images per batch (got %d)", n);
  if (n == 0) return LMKD_OK;
  LMKD_REQUIRE(data && descs && pool && status && trailer && out && scratch, "lmkd_png_decode: null pointer");
  LMKD_REQUIRE(((uintptr_t)data & 3) == 0 && aligned16(scratch), "lmkd_png_decode: data must be 4-byte, scratch 16-byte aligned");
  LMKD_REQUIRE(max_stride >= 0 && max_stride <= 4LL * PNG_MAX_DIM, "lmkd_png_decode: max_stride %lld outside 0 .. %d", max_stride,
               4 * PNG_MAX_DIM);
  hipStream_t s = (hipStream_t)stream;
  const PngDesc* D = (const PngDesc*)descs;
  hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(64), 0, s, data, D, scratch, status, trailer);
  LMKD_CHECK_LAUNCH("lmkd_png_decode (inflate)");
  const int rowcap = (int)align16ll(max_stride + 1);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(64), 3 * (size_t)rowcap, s, D, (const uint8_t*)pool, (const uint8_t*)scratch, out,
                     status, (const unsigned*)trailer, rowcap);
  LMKD_CHECK_LAUNCH("lmkd_png_decode (unfilter)");
  return LMKD_OK;
}

extern "C" int lmkd_png_decode_host(const unsigned char* data, const void* descs, const void* pool, int n, unsigned char* scratch,
                                    unsigned char* out, int* status) {
  LMKD_REQUIRE(n >= 0, "lmkd_png_decode_host: n < 0");
  const PngDesc* D = (const PngDesc*)descs;
  std::vector<uint8_t> rows;
  for (int i = 0; i < n; ++i) {
    const PngDesc& d = D[i];
    status[i] = PE_OK;
    if (d.kind != 0) continue;
    rows.assign(2 * (size_t)d.stride, 0);
    status[i] = decode_image_host(data, d.sb, d.se, d.W, d.H, d.ctype, d.bpp, d.stride, (const uint8_t*)pool + (d.ctype == 3 ? d.pal_off : 0),
                                  scratch + d.scr_off, rows.data(), out + d.out_off);
  }
  return LMKD_OK;
}
