// Baseline JPEG decoding: the frames of the reference's data trees (video_reader.py:118-196 read_dir, :334-343
// read_single_image = PIL.Image.open(f).load(), i.e. libjpeg-turbo with its defaults) decoded bit for bit on the GPU.
//
//   lmkd_jpeg_plan          host: parses and validates every header of a batch, builds one descriptor per image and a pool of
//                           derived tables (identical tables stored once), and says per image: decoded here, unsupported (the
//                           caller decodes it with PIL) or malformed
//   lmkd_jpeg_decode        three launches on the caller's stream:
//                             1. entropy decode, one wave per image: the wave copies the next window of compressed bytes into LDS,
//                                lane 0 decodes MCUs from it with the image's Huffman tables (also in LDS) into an LDS staging
//                                area, the wave writes the staged blocks out as int16 [block][64] in natural order
//                             2. dequantise + libjpeg's integer "islow" IDCT, eight lanes per block (columns, then rows)
//                             3. libjpeg's "fancy" upsampling of the chroma planes + YCbCr -> RGB into uint8 [H][W][3]
//   lmkd_jpeg_decode_host   the same per-block routines on the CPU (the tests' reference; not on the training path)
//   lmkd_jpeg_decode_host_windowed   the same, with launch 1's own program (window, refill, staging, flush) run lane by lane on the CPU
//
// The routines themselves are in jpeg_core.h, which also compiles as plain C++ (tools/jpeg_host_check.cpp).
// Everything in a file is outside input: every byte read is clamped to the image's scan range (reads past it return zero bits,
// as in libjpeg, and are reported), coefficient writes go to blocks the header's block count bounds, every loop is bounded by
// blocks x 64 symbols, and a bad code stops its own image only (status word).  Plain HIP C++, no inline assembly.
#include "common.h"
#include "jpeg_core.h"
#include <vector>

namespace {
using namespace jpegcore;

__constant__ unsigned char c_zz[64] = JPEG_ZZ;      // copied into LDS by the entropy kernel: a lookup per coefficient

// ---------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------
// a lane of the wave in jpegcore::entropy_windowed: its own iteration of every lane loop, the workgroup barrier between the phases
struct WaveDev {
  enum { COUNT = 1 };
  static __device__ __forceinline__ int first() { return (int)threadIdx.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const unsigned char* __restrict__ data, const JpegDesc* __restrict__ descs,
                                                          const unsigned char* __restrict__ pool, short* __restrict__ coef,
                                                          int* __restrict__ status) {
  __shared__ __align__(16) unsigned char win[EWIN];
  __shared__ __align__(16) short stage[ESTAGE * 64];
  __shared__ __align__(16) HuffTab tabs[6];
  __shared__ long long s_dest[ESTAGE];
  __shared__ unsigned char s_zz[64];
  __shared__ EntropyShared sh;
  const JpegDesc* dp = descs + blockIdx.x;
  if (dp->kind != 0) {
    if (threadIdx.x == 0) status[blockIdx.x] = JE_OK;
    return;
  }
  int pred[3];                            // the DC predictors: this kernel's own array (see entropy_windowed)
  const int err = entropy_windowed<WaveDev>(data, dp, pool, coef, win, stage, tabs, s_dest, s_zz, c_zz, &sh, pred);
  if (threadIdx.x == 0) status[blockIdx.x] = err;
}

// 32 blocks per workgroup, 8 lanes per block: lane c runs pass 1 on column c, then pass 2 on row c
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegDesc* __restrict__ descs, const unsigned char* __restrict__ pool,
                                                        const short* __restrict__ coef, unsigned char* __restrict__ planes) {
  __shared__ int ws[32][64];
  const JpegDesc& d = descs[blockIdx.y];
  if (d.kind != 0 || (long long)blockIdx.x * 32 >= d.nblocks) return;
  const int lb = blockIdx.x * 32 + (threadIdx.x >> 3), c = threadIdx.x & 7;
  const bool active = lb < d.nblocks;
  const int comp = lb >= d.comp_off[2] ? 2 : lb >= d.comp_off[1] ? 1 : 0;
  const long long gb = d.coef_off + lb;
  if (active) idct_col(coef + gb * 64, (const uint16_t*)(pool + d.qtab[comp]), c, ws[threadIdx.x >> 3]);
  __syncthreads();
  if (active) {
    unsigned char o[8];
    idct_row(&ws[threadIdx.x >> 3][c * 8], o);
    uint2 v;
    v.x = o[0] | (o[1] << 8) | (o[2] << 16) | ((unsigned)o[3] << 24);
    v.y = o[4] | (o[5] << 8) | (o[6] << 16) | ((unsigned)o[7] << 24);
    *(uint2*)(planes + gb * 64 + c * 8) = v;
  }
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegDesc* __restrict__ descs, const unsigned char* __restrict__ planes,
                                                         unsigned char* __restrict__ out) {
  const JpegDesc& d = descs[blockIdx.y];
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  if (d.kind != 0 || pix >= (long long)d.width * d.height) return;
  const int y = (int)(pix / d.width), x = (int)(pix - (long long)y * d.width);
  jpeg_pixel(planes + d.coef_off * 64, d, y, x, out + d.out_off + pix * 3);
}

}  // namespace

extern "C" long lmkd_jpeg_desc_bytes(void) { return (long)sizeof(JpegDesc); }

extern "C" long lmkd_jpeg_pool_bytes(int n) { return pool_bytes(n); }

extern "C" const char* lmkd_jpeg_reason(int reason) { return reason_text(reason); }

extern "C" int lmkd_jpeg_plan(const unsigned char* data, const long long* offsets, int n, void* descs, void* pool, long pool_cap,
                              long long* info, long long* totals) {
  LMKD_REQUIRE(n >= 0 && n <= 65535, "lmkd_jpeg_plan: 0 <= n <= 65535 images per batch (got %d)", n);
  LMKD_REQUIRE(totals && (n == 0 || (data && offsets && descs && pool && info)), "lmkd_jpeg_plan: null pointer");
  for (int i = 0; i < n; ++i)
    LMKD_REQUIRE(offsets[i] >= 0 && offsets[i + 1] >= offsets[i], "lmkd_jpeg_plan: offsets must be non-decreasing (image %d)", i);
  PoolEntries entries;
  long used = 0;
  long long blocks = 0, out_bytes = 0, max_blocks = 0, max_pixels = 0;
  JpegDesc* D = (JpegDesc*)descs;
  std::vector<Parsed> holder(1);
  Parsed& P = holder[0];
  for (int i = 0; i < n; ++i) {
    const long long b = offsets[i], e = offsets[i + 1];
    P = Parsed();
    int reason = JR_NONE;
    const int verdict = parse_jpeg(data + b, e - b, P, reason);
    JpegDesc& d = D[i];
    memset(&d, 0, sizeof d);
    d.kind = 1;
    info[5 * i + 0] = verdict;
    info[5 * i + 1] = reason;
    info[5 * i + 2] = verdict == JST_MALFORMED ? 0 : P.height;
    info[5 * i + 3] = verdict == JST_MALFORMED ? 0 : P.width;
    info[5 * i + 4] = out_bytes;
    if (verdict == JST_MALFORMED) continue;
    d.out_off = out_bytes;                 // an unsupported image keeps this descriptor (kind 1); plan_image writes a supported one anew
    const long long out_off = out_bytes;
    out_bytes += (long long)P.height * P.width * 3;
    if (verdict != JST_OK) continue;
    LMKD_REQUIRE(plan_image(P, b, out_off, blocks, d, entries, (unsigned char*)pool, pool_cap, used),
                 "lmkd_jpeg_plan: table pool of %ld bytes too small (lmkd_jpeg_pool_bytes)", pool_cap);
    blocks += d.nblocks;
    if (d.nblocks > max_blocks) max_blocks = d.nblocks;
    if ((long long)d.width * d.height > max_pixels) max_pixels = (long long)d.width * d.height;
  }
  totals[0] = used;
  totals[1] = blocks;
  totals[2] = out_bytes;
  totals[3] = max_blocks;
  totals[4] = max_pixels;
  return LMKD_OK;
}

extern "C" int lmkd_jpeg_decode(const unsigned char* data, const void* descs, const void* pool, int n, short* coef, unsigned char* planes,
                                unsigned char* out, int* status, long long max_blocks, long long max_pixels, void* stream) {
  LMKD_REQUIRE(n >= 0 && n <= 65535, "lmkd_jpeg_decode: 0 <= n <= 65535 images per batch (got %d)", n);
  if (n == 0) return LMKD_OK;
  LMKD_REQUIRE(data && descs && pool && status && out && coef && planes, "lmkd_jpeg_decode: null pointer");
  LMKD_REQUIRE(((uintptr_t)data & 3) == 0 && aligned16(pool) && aligned16(coef) && ((uintptr_t)planes & 7) == 0,
               "lmkd_jpeg_decode: data must be 4-byte, pool / coef 16-byte, planes 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const JpegDesc* D = (const JpegDesc*)descs;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n), dim3(64), 0, s, data, D, (const unsigned char*)pool, coef, status);
  LMKD_CHECK_LAUNCH("lmkd_jpeg_decode (entropy)");
  if (max_blocks > 0 && max_pixels > 0) {
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 31) / 32), n), dim3(256), 0, s, D, (const unsigned char*)pool,
                       (const short*)coef, planes);
    LMKD_CHECK_LAUNCH("lmkd_jpeg_decode (idct)");
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_pixels + 255) / 256), n), dim3(256), 0, s, D, (const unsigned char*)planes,
                       out);
    LMKD_CHECK_LAUNCH("lmkd_jpeg_decode (colour)");
  }
  return LMKD_OK;
}

extern "C" int lmkd_jpeg_decode_host(const unsigned char* data, const void* descs, const void* pool, int n, short* coef, unsigned char* planes,
                                     unsigned char* out, int* status) {
  LMKD_REQUIRE(n >= 0, "lmkd_jpeg_decode_host: n < 0");
  if (n == 0) return LMKD_OK;
  LMKD_REQUIRE(data && descs && pool && status && out && coef && planes, "lmkd_jpeg_decode_host: null pointer");
  const JpegDesc* D = (const JpegDesc*)descs;
  for (int i = 0; i < n; ++i) {
    const JpegDesc& d = D[i];
    status[i] = JE_OK;
    if (d.kind != 0) continue;
    status[i] = entropy_flat(data, d, (const unsigned char*)pool, coef);
    idct_color_host(d, (const unsigned char*)pool, coef, planes, out);
  }
  return LMKD_OK;
}

extern "C" int lmkd_jpeg_decode_host_windowed(const unsigned char* data, const void* descs, const void* pool, int n, short* coef,
                                              unsigned char* planes, unsigned char* out, int* status) {
  LMKD_REQUIRE(n >= 0, "lmkd_jpeg_decode_host_windowed: n < 0");
  if (n == 0) return LMKD_OK;
  LMKD_REQUIRE(data && descs && pool && status && out && coef && planes, "lmkd_jpeg_decode_host_windowed: null pointer");
  LMKD_REQUIRE(((uintptr_t)data & 3) == 0 && aligned16(pool) && aligned16(coef),
               "lmkd_jpeg_decode_host_windowed: data must be 4-byte, pool / coef 16-byte aligned (as for lmkd_jpeg_decode)");
  const JpegDesc* D = (const JpegDesc*)descs;
  for (int i = 0; i < n; ++i) {
    const JpegDesc& d = D[i];
    status[i] = JE_OK;
    if (d.kind != 0) continue;
    status[i] = entropy_windowed_host(data, d, (const unsigned char*)pool, coef);
    idct_color_host(d, (const unsigned char*)pool, coef, planes, out);
  }
  return LMKD_OK;
}
