// Baseline JPEG decoding routines shared by the GPU kernels and their host twins (csrc/jpeg.hip).  This header also compiles
// as plain C++ (tools/jpeg_host_check.cpp builds it without HIP): the qualifiers sit behind JPEG_HD.
//
// Everything in a file is outside input: every byte read is clamped to the image's scan range (reads past it return zero bits, as in
// libjpeg, and are reported), coefficient writes go to blocks the header's block count bounds, every loop is bounded by blocks x 64
// symbols, and a bad code stops its own image only (status word).  Plain C++, no inline assembly.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>

#ifndef JPEG_HD
#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif
#endif

namespace jpegcore {

#if defined(__HIPCC__)
typedef uint4 V16;                        // the 16-byte unit of the wave-wide copies
#else
struct alignas(16) V16 {
  uint32_t x, y, z, w;
};
#endif
JPEG_HD V16 v16_zero() {
  V16 v;
  v.x = v.y = v.z = v.w = 0;
  return v;
}

constexpr int JPEG_MAX_DIM = 4096;
constexpr int HLOOK = 9;                  // lookahead bits of the fast Huffman table

// libjpeg's derived decoding table (jdhuff.c jpeg_make_d_derived_tbl) + a 9-bit lookahead table
struct HuffTab {
  uint16_t look[1 << HLOOK];              // (code length << 8) | symbol for codes of <= 9 bits; 0 = longer code
  int32_t maxcode[18];                    // largest code of each length, -1 if none; [17] = sentinel
  int32_t valoff[18];                     // huffval index - code, per length
  uint8_t huffval[256];
};
static_assert(sizeof(HuffTab) % 16 == 0, "HuffTab is copied in 16-byte units");

struct QTab {
  uint16_t q[64];                         // natural order
};
static_assert(sizeof(QTab) % 16 == 0, "the pool keeps every table 16-byte aligned");

struct JpegDesc {
  long long scan_begin, scan_end;         // entropy-coded bytes [scan_begin, scan_end) of the packed input; scan_end = the 0xFF of the
                                          // marker that ends the scan (scan_end + 1 < end of the image's bytes)
  long long out_off;                      // byte offset of the image's uint8 [H][W][3] in the output
  long long coef_off;                     // first block of the image in the coefficient / sample-plane scratch
  int kind;                               // 0 = decoded by lmkd_jpeg_decode, 1 = not (the caller fills the slot or raises)
  int width, height;
  int hs, vs;                             // luma sampling factors; chroma is 1x1
  int mcux, mcuy;
  int restart;                            // restart interval in MCUs, 0 = none
  int nblocks;                            // blocks of the image (all three planes)
  int comp_off[3];                        // first block of each component plane, relative to coef_off
  int bw[3];                              // blocks per row of each plane (rows: mcuy * v)
  int dw[3], dh[3];                       // real samples of each plane (libjpeg's downsampled_width / _height)
  int qtab[3];                            // byte offsets into the table pool
  int dctab[3], actab[3];
  int pad_;
};
static_assert(sizeof(JpegDesc) % 8 == 0, "descriptor array");

// plan verdicts (info[0]) and reasons (info[1])
enum { JST_OK = 0, JST_UNSUPPORTED = 1, JST_MALFORMED = 2 };
enum {
  JR_NONE = 0,
  JR_PROGRESSIVE = 1, JR_ARITHMETIC = 2, JR_SOF_OTHER = 3, JR_COMPONENTS = 4, JR_SAMPLING = 5, JR_COLOR = 6, JR_QT16 = 7,
  JR_SCANS = 8, JR_SIZE = 9, JR_MARKER = 10,
  JR_NO_SOI = 20, JR_TRUNCATED = 21, JR_SEGMENT = 22, JR_TABLE_ID = 23, JR_HUFF = 24, JR_UNDEFINED = 25, JR_SCAN = 26,
  JR_NO_SCAN_END = 27, JR_FRAME = 28, JR_NO_FRAME = 29,
};
// device status words
enum { JE_OK = 0, JE_BADCODE = 1, JE_COEF = 2, JE_PAST_END = 3, JE_RESTART = 4, JE_TRAILING = 5, JE_WINDOW = 6 };

#define JPEG_ZZ                                                                                                                   \
  { 0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 }
static const unsigned char h_zz[64] = JPEG_ZZ;      // the host's copy (the kernel's lies in constant memory, csrc/jpeg.hip)

// ---------------------------------------------------------------------------------------------------------------------------
// entropy decoding (jdhuff.c), shared by the kernel and the host entries
// ---------------------------------------------------------------------------------------------------------------------------
struct BitState {
  unsigned long long acc;                 // the low `nbits` bits are unconsumed
  int nbits, pad;                         // pad: zero bits appended after the scan's end marker (libjpeg's behaviour)
  int marker;                             // the reader has reached a marker
  int err;
  long long pos;                          // next byte
};

template <class Src>
JPEG_HD void fill_bits(BitState& s, const Src& src, long long scan_end) {
  while (s.nbits <= 56) {
    if (s.marker || s.pos >= scan_end) {
      s.marker = 1;
      s.acc <<= 8;
      s.nbits += 8;
      s.pad += 8;
      continue;
    }
    int b = src.byte(s.pos);
    if (b == 0xFF) {
      int nb = (s.pos + 1 < scan_end) ? src.byte(s.pos + 1) : 0xFF;
      if (nb != 0) {                      // a marker (RSTn, or fill bytes in front of one): no more data in this interval
        s.marker = 1;
        continue;
      }
      s.pos += 2;                         // stuffed 0xFF 0x00
    } else {
      s.pos += 1;
    }
    s.acc = (s.acc << 8) | (unsigned)b;
    s.nbits += 8;
  }
}

// needs nbits >= 16 (fill_bits leaves > 56)
JPEG_HD int huff_decode(BitState& s, const HuffTab& h) {
  unsigned peek = (unsigned)(s.acc >> (s.nbits - HLOOK)) & ((1u << HLOOK) - 1);
  int e = h.look[peek];
  if (e >> 8) {
    s.nbits -= e >> 8;
    return e & 255;
  }
  for (int l = HLOOK + 1; l <= 16; ++l) {
    int code = (int)((s.acc >> (s.nbits - l)) & ((1ull << l) - 1));
    if (code <= h.maxcode[l]) {
      s.nbits -= l;
      return h.huffval[(code + h.valoff[l]) & 255];
    }
  }
  return -1;
}

JPEG_HD int get_extend(BitState& s, int n) {      // n in 1..15
  s.nbits -= n;
  int v = (int)((s.acc >> s.nbits) & ((1u << n) - 1));
  return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// one 8x8 block: DC difference + AC run/size symbols (jdhuff.c decode_mcu_slow); blk must be zero on entry
template <class Src>
JPEG_HD void decode_block(BitState& s, const Src& src, long long scan_end, const HuffTab& dc, const HuffTab& ac, const unsigned char* zz,
                          int& pred, short* blk) {
  fill_bits(s, src, scan_end);
  int t = huff_decode(s, dc);
  if (t < 0 || t > 15) {
    s.err = JE_BADCODE;
    return;
  }
  int diff = t ? get_extend(s, t) : 0;
  pred = (int)((unsigned)pred + (unsigned)diff);
  blk[0] = (short)pred;
  for (int k = 1; k < 64; ++k) {
    fill_bits(s, src, scan_end);
    int rs = huff_decode(s, ac);
    if (rs < 0) {
      s.err = JE_BADCODE;
      return;
    }
    int r = rs >> 4, sz = rs & 15;
    if (sz) {
      k += r;
      if (k > 63) {
        s.err = JE_COEF;
        return;
      }
      blk[zz[k]] = (short)get_extend(s, sz);
    } else {
      if (r != 15) break;                 // EOB
      k += 15;                            // ZRL
    }
  }
}

// the end of a restart interval (final = false) or of the scan: at most the padding bits of the last byte are left, then the
// expected RSTn (or, at the end, only fill bytes up to the marker that ends the scan)
template <class Src>
JPEG_HD void end_interval(BitState& s, const Src& src, long long scan_end, int& rst, bool final) {
  int real = s.nbits - s.pad;
  if (real < 0) {
    s.err = JE_PAST_END;
    return;
  }
  if (real >= 8) {
    s.err = JE_TRAILING;
    return;
  }
  long long p = s.pos;
  if (final) {
    while (p < scan_end && src.byte(p) == 0xFF) ++p;
    if (p != scan_end) s.err = JE_TRAILING;
    return;
  }
  while (p + 1 < scan_end && src.byte(p) == 0xFF && src.byte(p + 1) == 0xFF) ++p;
  if (!(p + 1 < scan_end && src.byte(p) == 0xFF && src.byte(p + 1) == 0xD0 + (rst & 7))) {
    s.err = JE_RESTART;
    return;
  }
  s.pos = p + 2;
  s.acc = 0;
  s.nbits = s.pad = s.marker = 0;
  ++rst;
}

// MCU `mcu` of the interleaved scan; sink(comp, block row, block column) -> zeroed short[64] for the block
template <class Src, class Sink>
JPEG_HD void decode_mcu(const JpegDesc& d, const HuffTab* tabs, const unsigned char* zz, BitState& s, const Src& src, int* pred,
                        long long mcu, int& rst, Sink& sink) {
  if (d.restart && mcu > 0 && mcu % d.restart == 0) {
    end_interval(s, src, d.scan_end, rst, false);
    if (s.err) return;
    pred[0] = pred[1] = pred[2] = 0;
  }
  const int my = (int)(mcu / d.mcux), mx = (int)(mcu - (long long)my * d.mcux);
  for (int yy = 0; yy < d.vs; ++yy)
    for (int xx = 0; xx < d.hs; ++xx) {
      decode_block(s, src, d.scan_end, tabs[0], tabs[3], zz, pred[0], sink(0, my * d.vs + yy, mx * d.hs + xx));
      if (s.err) return;
    }
  for (int c = 1; c < 3; ++c) {
    decode_block(s, src, d.scan_end, tabs[c], tabs[3 + c], zz, pred[c], sink(c, my, mx));
    if (s.err) return;
  }
  if (s.nbits < s.pad) s.err = JE_PAST_END;
}

// ---------------------------------------------------------------------------------------------------------------------------
// jidctint.c jpeg_idct_islow: pass 1 on the columns (dequantised), pass 2 on the rows; output range_limit[x & 1023] centred at 128
// ---------------------------------------------------------------------------------------------------------------------------
#define FIX_0_298631336 2446LL
#define FIX_0_390180644 3196LL
#define FIX_0_541196100 4433LL
#define FIX_0_765366865 6270LL
#define FIX_0_899976223 7373LL
#define FIX_1_175875602 9633LL
#define FIX_1_501321110 12299LL
#define FIX_1_847759065 15137LL
#define FIX_1_961570560 16069LL
#define FIX_2_053119869 16819LL
#define FIX_2_562915447 20995LL
#define FIX_3_072711026 25172LL

JPEG_HD long long descale(long long x, int n) { return (x + (1LL << (n - 1))) >> n; }

// libjpeg's idct_sample_range_limit table for 8-bit samples, index v & 1023
JPEG_HD unsigned char idct_limit(long long v) {
  int t = (int)(v & 1023);
  return (unsigned char)(t < 128 ? t + 128 : t < 512 ? 255 : t < 896 ? 0 : t - 896);
}

// the butterfly both passes share (even part, then odd part; i0..i3 = z7, z5, z3, z1), before descaling
JPEG_HD void idct_1d(long long z0, long long z1, long long z2, long long z3, long long z4, long long z5, long long z6, long long z7,
                     long long* o) {
  long long a = (z2 + z6) * FIX_0_541196100;
  long long tmp2 = a + z6 * -FIX_1_847759065;
  long long tmp3 = a + z2 * FIX_0_765366865;
  long long tmp0 = (z0 + z4) * 8192;      // LEFT_SHIFT(.., CONST_BITS)
  long long tmp1 = (z0 - z4) * 8192;
  const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = z7;
  tmp1 = z5;
  tmp2 = z3;
  tmp3 = z1;
  long long q1 = tmp0 + tmp3, q2 = tmp1 + tmp2, q3 = tmp0 + tmp2, q4 = tmp1 + tmp3;
  const long long q5 = (q3 + q4) * FIX_1_175875602;
  tmp0 = tmp0 * FIX_0_298631336;
  tmp1 = tmp1 * FIX_2_053119869;
  tmp2 = tmp2 * FIX_3_072711026;
  tmp3 = tmp3 * FIX_1_501321110;
  q1 = q1 * -FIX_0_899976223;
  q2 = q2 * -FIX_2_562915447;
  q3 = q3 * -FIX_1_961570560;
  q4 = q4 * -FIX_0_390180644;
  q3 += q5;
  q4 += q5;
  tmp0 += q1 + q3;
  tmp1 += q2 + q4;
  tmp2 += q2 + q3;
  tmp3 += q1 + q4;
  o[0] = tmp10 + tmp3;
  o[7] = tmp10 - tmp3;
  o[1] = tmp11 + tmp2;
  o[6] = tmp11 - tmp2;
  o[2] = tmp12 + tmp1;
  o[5] = tmp12 - tmp1;
  o[3] = tmp13 + tmp0;
  o[4] = tmp13 - tmp0;
}

// pass 1, column c of a block: ws[r * 8 + c]
JPEG_HD void idct_col(const short* blk, const uint16_t* q, int c, int* ws) {
  long long z[8];
  for (int r = 0; r < 8; ++r) z[r] = (long long)blk[r * 8 + c] * (long long)q[r * 8 + c];
  if (z[1] == 0 && z[2] == 0 && z[3] == 0 && z[4] == 0 && z[5] == 0 && z[6] == 0 && z[7] == 0) {
    const int dc = (int)(z[0] * 4);       // LEFT_SHIFT(.., PASS1_BITS)
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = dc;
    return;
  }
  long long o[8];
  idct_1d(z[0], z[1], z[2], z[3], z[4], z[5], z[6], z[7], o);
  for (int r = 0; r < 8; ++r) ws[r * 8 + c] = (int)descale(o[r], 11);
}

// pass 2, one row (8 workspace values) -> 8 samples
JPEG_HD void idct_row(const int* w, unsigned char* out) {
  if (w[1] == 0 && w[2] == 0 && w[3] == 0 && w[4] == 0 && w[5] == 0 && w[6] == 0 && w[7] == 0) {
    const unsigned char v = idct_limit(descale((long long)w[0], 5));
    for (int i = 0; i < 8; ++i) out[i] = v;
    return;
  }
  long long o[8];
  idct_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], o);
  for (int i = 0; i < 8; ++i) out[i] = idct_limit(descale(o[i], 18));
}

// ---------------------------------------------------------------------------------------------------------------------------
// jdsample.c fancy upsampling (h2v1 / h2v2, only for planes wider than 2 samples; box replication otherwise) + jdcolor.c
// ycc_rgb_convert, one output pixel
// ---------------------------------------------------------------------------------------------------------------------------
JPEG_HD int plane_at(const unsigned char* pl, const JpegDesc& d, int c, int r, int x) {
  return pl[((long long)d.comp_off[c] + (long long)(r >> 3) * d.bw[c] + (x >> 3)) * 64 + (r & 7) * 8 + (x & 7)];
}

JPEG_HD int chroma_at(const unsigned char* pl, const JpegDesc& d, int c, int y, int x) {
  if (d.hs == 1) return plane_at(pl, d, c, y, x);                     // 4:4:4 (vs == 1 too)
  const int dw = d.dw[c], dh = d.dh[c];
  const int cc = x >> 1;
  if (dw <= 2) return plane_at(pl, d, c, d.vs == 2 ? y >> 1 : y, cc);  // h2v1_upsample / h2v2_upsample
  const int side = (x & 1) ? (cc + 1 < dw ? cc + 1 : dw - 1) : (cc > 0 ? cc - 1 : 0);
  if (d.vs == 1) {                                                    // h2v1_fancy_upsample
    const int v = 3 * plane_at(pl, d, c, y, cc) + plane_at(pl, d, c, y, side);
    return (x & 1) ? (v + 2) >> 2 : (v + 1) >> 2;
  }
  const int r = y >> 1;                                               // h2v2_fancy_upsample
  const int rn = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
  const int s0 = 3 * plane_at(pl, d, c, r, cc) + plane_at(pl, d, c, rn, cc);
  const int s1 = 3 * plane_at(pl, d, c, r, side) + plane_at(pl, d, c, rn, side);
  return (x & 1) ? (3 * s0 + s1 + 7) >> 4 : (3 * s0 + s1 + 8) >> 4;
}

JPEG_HD unsigned char clamp255(int v) { return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v); }

JPEG_HD void jpeg_pixel(const unsigned char* pl, const JpegDesc& d, int y, int x, unsigned char* rgb) {
  const int Y = plane_at(pl, d, 0, y, x);
  const int cb = chroma_at(pl, d, 1, y, x) - 128, cr = chroma_at(pl, d, 2, y, x) - 128;
  rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  rgb[1] = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

// ---------------------------------------------------------------------------------------------------------------------------
// the entropy decode of one image by a wave (launch 1 of lmkd_jpeg_decode): compressed bytes through a window, blocks through a
// staging area.  Lane 0 runs the serial decoder; what the wave does in parallel stands in loops over the lanes, JPEG_LANES(t)
// (the Wv::COUNT lanes a thread runs, from Wv::first() on), and Wv::sync() separates the phases.  On the GPU a lane runs its own
// iteration and sync is the workgroup barrier; WaveSim runs the 64 lanes one after the other on one thread, which is the same
// program in plain C++ (tools/jpeg_host_check.cpp runs it under the sanitizers with win, stage, tabs and dest as heap blocks of
// exactly these sizes).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int EWIN = 8192;                // window of compressed bytes
constexpr int EGUARD = 3328;              // refill when fewer bytes than this are left in the window: one MCU reads at most
                                          // 6 blocks x 64 x (16 + 15) bits, doubled by byte stuffing = 2976 bytes, + lookahead
constexpr int ESTAGE = 48;                // staged blocks (8 MCUs of 6 blocks)

#define JPEG_LANES(t) for (int t = Wv::first(), t##_k = 0; t##_k < Wv::COUNT; ++t##_k, ++t)

struct WaveSim {
  enum { COUNT = 64 };
  static int first() { return 0; }
  static void sync() {}
};

struct WinSrc {
  const unsigned char* win;
  long long base;
  mutable int over;
  JPEG_HD int byte(long long p) const {
    const long long o = p - base;
    if (o < 0 || o >= EWIN) {
      over = 1;
      return 0;
    }
    return win[o];
  }
};

struct StageSink {
  short* stage;
  long long* dest;
  const JpegDesc* d;
  int n;
  JPEG_HD short* operator()(int c, int by, int bx) {
    dest[n] = d->coef_off + d->comp_off[c] + (long long)by * d->bw[c] + bx;
    return stage + 64 * n++;
  }
};

// what lane 0 tells the wave after each round
struct EntropyShared {
  long long win;                          // position of win[0] in `data`, a multiple of 4
  int nst, done, refill;                  // staged blocks to write out; the image is finished (or stopped); fill the window again
};

// data: the packed input (4-byte aligned; the image's bytes from scan_begin & ~3 to scan_end + 2 are readable); *dp: the image's
// descriptor (kind 0); pool, coef: 16-byte aligned.  win: EWIN bytes, stage: ESTAGE x 64 shorts, tabs: 6 tables, dest: ESTAGE words,
// zz: 64 bytes (filled here from zz_src), sh: one EntropyShared - all of them the wave's own (LDS on the GPU), 16-byte aligned.
// pred: the three DC predictors, an array of the caller's own.  It is the caller's because of how the kernel compiles: an array
// that belongs to the kernel itself is turned into one three-word register value when this body has been inlined there; as a
// local of this function it is split into three scalars before that, and the entropy launch then took 1.3 % longer.
// -> the image's status word (lane 0's value is the one that counts)
template <class Wv>
JPEG_HD int entropy_windowed(const unsigned char* data, const JpegDesc* dp, const unsigned char* pool, short* coef, unsigned char* win,
                             short* stage, HuffTab* tabs, long long* dest, unsigned char* zz, const unsigned char* zz_src,
                             EntropyShared* sh, int* pred) {
  const JpegDesc d = *dp;
  JPEG_LANES(t) {
    for (int k = 0; k < 6; ++k) {
      const V16* src = (const V16*)(pool + (k < 3 ? d.dctab[k] : d.actab[k - 3]));
      V16* dst = (V16*)&tabs[k];
      for (int i = t; i < (int)(sizeof(HuffTab) / 16); i += 64) dst[i] = src[i];
    }
    for (int i = t; i < ESTAGE * 8; i += 64) ((V16*)stage)[i] = v16_zero();
    zz[t] = zz_src[t];
  }
  if (Wv::first() == 0) {
    sh->win = d.scan_begin & ~3LL;
    sh->refill = 1;
    sh->done = 0;
  }
  Wv::sync();
  BitState st = {0ull, 0, 0, 0, 0, d.scan_begin};
  pred[0] = pred[1] = pred[2] = 0;
  int rst = 0;
  long long mcu = 0;
  const long long total = (long long)d.mcux * d.mcuy;
  const long long lim = d.scan_end + 2;   // the window also holds the end marker's two bytes
  const int per_mcu = d.hs * d.vs + 2;
  for (;;) {
    if (sh->refill) {
      const long long base = sh->win;
      const long long n = (lim - base < EWIN) ? lim - base : EWIN;
      const unsigned char* g = data + base;
      const int nd = (int)(n >> 2);
      JPEG_LANES(t) {
        for (int i = t; i < nd; i += 64) ((uint32_t*)win)[i] = ((const uint32_t*)g)[i];
        for (int i = nd * 4 + t; i < n; i += 64) win[i] = g[i];
      }
    }
    Wv::sync();
    if (Wv::first() == 0) {
      const long long base = sh->win;
      WinSrc src{win, base, 0};
      StageSink sink{stage, dest, dp, 0};
      const bool covers_end = base + EWIN >= lim;
      while (mcu < total && !st.err && sink.n + per_mcu <= ESTAGE && (covers_end || st.pos - base <= EWIN - EGUARD)) {
        decode_mcu(d, tabs, zz, st, src, pred, mcu, rst, sink);
        ++mcu;
        if (src.over && !st.err) st.err = JE_WINDOW;
      }
      if (!st.err && mcu == total) {
        end_interval(st, src, d.scan_end, rst, true);
        if (src.over && !st.err) st.err = JE_WINDOW;
      }
      sh->nst = st.err ? 0 : sink.n;      // a failed image's partly decoded staging is dropped (and zeroed below)
      sh->done = (mcu == total || st.err) ? 1 : 0;
      const bool need = !sh->done && !covers_end && st.pos - base > EWIN - EGUARD;
      sh->refill = need ? 1 : 0;
      if (need) sh->win = st.pos & ~3LL;
    }
    Wv::sync();
    const int nst = sh->nst;
    JPEG_LANES(t)
      for (int i = t; i < nst * 8; i += 64) ((V16*)(coef + dest[i >> 3] * 64))[i & 7] = ((const V16*)(stage + (i >> 3) * 64))[i & 7];
    Wv::sync();
    JPEG_LANES(t)
      for (int i = t; i < ESTAGE * 8; i += 64) ((V16*)stage)[i] = v16_zero();
    const int done = sh->done;
    Wv::sync();
    if (done) break;
  }
  return st.err;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: header parsing (jdmarker.c), table derivation, the plan of one image, the flat decode
// ---------------------------------------------------------------------------------------------------------------------------
inline int be16(const unsigned char* p) { return (p[0] << 8) | p[1]; }

// jdhuff.c jpeg_make_d_derived_tbl; false on an over-subscribed code space or a DC symbol > 15
inline bool build_huff(const unsigned char* counts /*[17], [0] unused*/, const unsigned char* vals, bool dc, HuffTab& t) {
  memset(&t, 0, sizeof t);
  unsigned char size[257];
  unsigned code[257];
  int p = 0;
  for (int l = 1; l <= 16; ++l)
    for (int i = 0; i < counts[l]; ++i) size[p++] = (unsigned char)l;
  size[p] = 0;
  const int num = p;
  unsigned c = 0;
  int si = size[0];
  p = 0;
  while (size[p]) {
    while (size[p] == si) code[p++] = c++;
    if (c >= (1u << si)) return false;
    c <<= 1;
    ++si;
  }
  p = 0;
  for (int l = 1; l <= 16; ++l) {
    if (counts[l]) {
      t.valoff[l] = p - (int)code[p];
      p += counts[l];
      t.maxcode[l] = (int)code[p - 1];
    } else {
      t.maxcode[l] = -1;
    }
  }
  t.maxcode[17] = 0xFFFFF;
  p = 0;
  for (int l = 1; l <= HLOOK; ++l)
    for (int i = 0; i < counts[l]; ++i, ++p) {
      const int look = (int)code[p] << (HLOOK - l);
      for (int k = 0; k < (1 << (HLOOK - l)); ++k) t.look[look + k] = (uint16_t)((l << 8) | vals[p]);
    }
  memcpy(t.huffval, vals, num);
  if (dc)
    for (int i = 0; i < num; ++i)
      if (vals[i] > 15) return false;
  return true;
}

struct Parsed {
  int width = 0, height = 0;
  int id[3] = {0, 0, 0}, h[3] = {0, 0, 0}, v[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
  int qdef[4] = {0, 0, 0, 0};
  uint16_t q[4][64];
  int hdef[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  unsigned char hcount[2][4][17];
  unsigned char hval[2][4][256];
  int restart = 0;
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  long long scan_begin = 0, scan_end = 0;
  int jfif = 0, adobe = 0;
  HuffTab dct[3], act[3];
};

// -> verdict; `reason`; fills P (the size also for unsupported files)
inline int parse_jpeg(const unsigned char* d, long long n, Parsed& P, int& reason) {
  reason = JR_NONE;
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return reason = JR_NO_SOI, JST_MALFORMED;
  long long pos = 2;
  bool have_sof = false;
  for (;;) {
    while (pos < n && d[pos] != 0xFF) ++pos;            // libjpeg skips (and warns about) garbage between segments
    while (pos < n && d[pos] == 0xFF) ++pos;            // fill bytes
    if (pos >= n) return reason = JR_TRUNCATED, JST_MALFORMED;
    const int m = d[pos++];
    if (m == 0 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;      // stuffed zero / parameterless markers outside a scan
    if (m == 0xD8) return reason = JR_NO_SOI, JST_MALFORMED;
    if (m == 0xD9) return reason = (have_sof ? JR_NO_SCAN_END : JR_NO_FRAME), JST_MALFORMED;
    if (pos + 2 > n) return reason = JR_TRUNCATED, JST_MALFORMED;
    const int L = be16(d + pos);
    if (L < 2) return reason = JR_SEGMENT, JST_MALFORMED;
    if (pos + L > n) return reason = JR_TRUNCATED, JST_MALFORMED;
    const unsigned char* s = d + pos + 2;
    const int len = L - 2;
    pos += L;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {          // SOFn
      if (have_sof) return reason = JR_FRAME, JST_MALFORMED;
      have_sof = true;
      if (len < 6) return reason = JR_SEGMENT, JST_MALFORMED;
      const int prec = s[0], nf = s[5];
      P.height = be16(s + 1);
      P.width = be16(s + 3);
      if (len != 6 + 3 * nf || nf == 0) return reason = JR_SEGMENT, JST_MALFORMED;
      if (P.width == 0) return reason = JR_FRAME, JST_MALFORMED;
      for (int i = 0; i < nf; ++i) {
        const int hv = s[7 + 3 * i];
        if ((hv >> 4) < 1 || (hv >> 4) > 4 || (hv & 15) < 1 || (hv & 15) > 4 || s[8 + 3 * i] > 3) return reason = JR_FRAME, JST_MALFORMED;
      }
      if (m == 0xC2) return reason = JR_PROGRESSIVE, JST_UNSUPPORTED;
      if (m >= 0xC9) return reason = JR_ARITHMETIC, JST_UNSUPPORTED;
      if (m != 0xC0) return reason = JR_SOF_OTHER, JST_UNSUPPORTED;
      if (prec != 8) return reason = JR_FRAME, JST_MALFORMED;
      if (P.height == 0 || P.width > JPEG_MAX_DIM || P.height > JPEG_MAX_DIM) return reason = JR_SIZE, JST_UNSUPPORTED;
      if (nf != 3) return reason = JR_COMPONENTS, JST_UNSUPPORTED;
      for (int i = 0; i < 3; ++i) {
        P.id[i] = s[6 + 3 * i];
        P.h[i] = s[7 + 3 * i] >> 4;
        P.v[i] = s[7 + 3 * i] & 15;
        P.tq[i] = s[8 + 3 * i];
      }
      if (P.id[0] == P.id[1] || P.id[0] == P.id[2] || P.id[1] == P.id[2]) return reason = JR_FRAME, JST_MALFORMED;
      const bool luma_ok = (P.h[0] == 1 && P.v[0] == 1) || (P.h[0] == 2 && P.v[0] == 1) || (P.h[0] == 2 && P.v[0] == 2);
      if (!luma_ok || P.h[1] != 1 || P.v[1] != 1 || P.h[2] != 1 || P.v[2] != 1) return reason = JR_SAMPLING, JST_UNSUPPORTED;
    } else if (m == 0xC4) {                                                         // DHT
      int k = 0;
      while (k < len) {
        const int tc = s[k] >> 4, th = s[k] & 15;
        if (tc > 1 || th > 3) return reason = JR_TABLE_ID, JST_MALFORMED;
        if (k + 17 > len) return reason = JR_SEGMENT, JST_MALFORMED;
        int count = 0;
        P.hcount[tc][th][0] = 0;
        for (int l = 1; l <= 16; ++l) count += (P.hcount[tc][th][l] = s[k + l]);
        if (count > 256 || k + 17 + count > len) return reason = JR_HUFF, JST_MALFORMED;
        memcpy(P.hval[tc][th], s + k + 17, count);
        P.hdef[tc][th] = 1;
        k += 17 + count;
      }
    } else if (m == 0xCC) {
      return reason = JR_ARITHMETIC, JST_UNSUPPORTED;
    } else if (m == 0xDB) {                                                         // DQT
      int k = 0;
      while (k < len) {
        const int pq = s[k] >> 4, tq = s[k] & 15;
        if (tq > 3) return reason = JR_TABLE_ID, JST_MALFORMED;
        if (pq == 1) return reason = JR_QT16, JST_UNSUPPORTED;
        if (pq != 0 || k + 65 > len) return reason = JR_SEGMENT, JST_MALFORMED;
        for (int i = 0; i < 64; ++i) P.q[tq][h_zz[i]] = s[k + 1 + i];
        P.qdef[tq] = 1;
        k += 65;
      }
    } else if (m == 0xDD) {                                                         // DRI
      if (len != 2) return reason = JR_SEGMENT, JST_MALFORMED;
      P.restart = be16(s);
    } else if (m == 0xDA) {                                                         // SOS
      if (!have_sof) return reason = JR_NO_FRAME, JST_MALFORMED;
      if (len < 1) return reason = JR_SEGMENT, JST_MALFORMED;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || len != 4 + 2 * ns) return reason = JR_SEGMENT, JST_MALFORMED;
      int seen = 0;
      for (int i = 0; i < ns; ++i) {
        int c = -1;
        for (int j = 0; j < 3; ++j)
          if (P.id[j] == s[1 + 2 * i]) c = j;
        if (c < 0 || ((seen >> c) & 1)) return reason = JR_SCAN, JST_MALFORMED;
        seen |= 1 << c;
        P.td[c] = s[2 + 2 * i] >> 4;
        P.ta[c] = s[2 + 2 * i] & 15;
        if (P.td[c] > 3 || P.ta[c] > 3) return reason = JR_TABLE_ID, JST_MALFORMED;
      }
      const int Ss = s[1 + 2 * ns], Se = s[2 + 2 * ns], AhAl = s[3 + 2 * ns];
      if (Ss != 0 || Se != 63 || AhAl != 0) return reason = JR_SCAN, JST_MALFORMED;
      if (ns != 3) return reason = JR_SCANS, JST_UNSUPPORTED;
      for (int c = 0; c < 3; ++c) {
        if (!P.qdef[P.tq[c]] || !P.hdef[0][P.td[c]] || !P.hdef[1][P.ta[c]]) return reason = JR_UNDEFINED, JST_MALFORMED;
        if (!build_huff(P.hcount[0][P.td[c]], P.hval[0][P.td[c]], true, P.dct[c]) ||
            !build_huff(P.hcount[1][P.ta[c]], P.hval[1][P.ta[c]], false, P.act[c]))
          return reason = JR_HUFF, JST_MALFORMED;
      }
      // the entropy-coded segment ends at the first marker other than RSTn (fill bytes 0xFF belong to the marker)
      P.scan_begin = pos;
      long long p = pos;
      int end_marker = -1;
      while (p < n) {
        const void* f = memchr(d + p, 0xFF, (size_t)(n - p));
        if (!f) break;
        p = (const unsigned char*)f - d;
        long long q = p + 1;
        while (q < n && d[q] == 0xFF) ++q;
        if (q >= n) break;
        const int c = d[q];
        if (c == 0 || (c >= 0xD0 && c <= 0xD7)) {
          p = q + 1;
          continue;
        }
        P.scan_end = q - 1;
        end_marker = c;
        break;
      }
      if (end_marker < 0) return reason = JR_NO_SCAN_END, JST_MALFORMED;
      if (end_marker != 0xD9) return reason = JR_SCANS, JST_UNSUPPORTED;         // more scans (or tables / DNL) follow
      if (P.adobe || !(P.jfif || (P.id[0] == 1 && P.id[1] == 2 && P.id[2] == 3))) return reason = JR_COLOR, JST_UNSUPPORTED;
      return JST_OK;
    } else if (m == 0xE0) {
      if (len >= 5 && memcmp(s, "JFIF\0", 5) == 0) P.jfif = 1;
    } else if (m == 0xEE) {
      if (len >= 5 && memcmp(s, "Adobe", 5) == 0) P.adobe = 1;
    } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE || m == 0xDC) {
      // APPn / COM / DNL outside a scan: skipped, as libjpeg does
    } else {
      return reason = JR_MARKER, JST_UNSUPPORTED;
    }
  }
}

inline const char* reason_text(int reason) {
  switch (reason) {
    case JR_NONE: return "supported";
    case JR_PROGRESSIVE: return "progressive";
    case JR_ARITHMETIC: return "arithmetic coding";
    case JR_SOF_OTHER: return "frame type other than baseline (SOF0)";
    case JR_COMPONENTS: return "component count other than 3";
    case JR_SAMPLING: return "sampling other than 4:4:4 / 4:2:2 / 4:2:0";
    case JR_COLOR: return "colour space other than YCbCr";
    case JR_QT16: return "16-bit quantisation table";
    case JR_SCANS: return "more than one scan";
    case JR_SIZE: return "size above 4096 or height from DNL";
    case JR_MARKER: return "unknown marker";
    case JR_NO_SOI: return "no SOI marker";
    case JR_TRUNCATED: return "truncated header";
    case JR_SEGMENT: return "bad segment";
    case JR_TABLE_ID: return "bad table id";
    case JR_HUFF: return "bad Huffman table";
    case JR_UNDEFINED: return "table referenced but never defined";
    case JR_SCAN: return "bad scan parameters";
    case JR_NO_SCAN_END: return "scan does not end in a marker inside the buffer";
    case JR_FRAME: return "bad frame header";
    case JR_NO_FRAME: return "no frame header before the scan";
    default: return "unknown";
  }
}

// bytes of the table pool that n images need at the most
inline long pool_bytes(int n) { return (long)(n > 0 ? n : 1) * (6 * (long)sizeof(HuffTab) + 3 * (long)sizeof(QTab)); }

// the table pool: byte offset of an identical entry, or of a new one (-1: the pool is full)
typedef std::vector<std::pair<long, long>> PoolEntries;
inline long pool_put(PoolEntries& entries, unsigned char* pool, long cap, long& used, const void* data, long bytes) {
  for (auto& e : entries)
    if (e.second == bytes && memcmp(pool + e.first, data, bytes) == 0) return e.first;
  if (used + bytes > cap) return -1;
  memcpy(pool + used, data, bytes);
  entries.push_back({used, bytes});
  used += bytes;
  return used - bytes;
}

// the descriptor of a supported image (verdict JST_OK) whose file begins at byte `b` of the packed input, and its tables into the pool;
// out_off / coef_off are the caller's running totals.  false: the pool is full
inline bool plan_image(const Parsed& P, long long b, long long out_off, long long coef_off, JpegDesc& d, PoolEntries& entries,
                       unsigned char* pool, long pool_cap, long& used) {
  memset(&d, 0, sizeof d);
  d.out_off = out_off;
  d.kind = 0;
  d.width = P.width;
  d.height = P.height;
  d.hs = P.h[0];
  d.vs = P.v[0];
  d.mcux = (d.width + 8 * d.hs - 1) / (8 * d.hs);
  d.mcuy = (d.height + 8 * d.vs - 1) / (8 * d.vs);
  d.restart = P.restart;
  d.scan_begin = b + P.scan_begin;
  d.scan_end = b + P.scan_end;
  int off = 0;
  for (int c = 0; c < 3; ++c) {
    d.comp_off[c] = off;
    d.bw[c] = d.mcux * P.h[c];
    off += d.bw[c] * d.mcuy * P.v[c];
    d.dw[c] = (d.width * P.h[c] + d.hs - 1) / d.hs;
    d.dh[c] = (d.height * P.v[c] + d.vs - 1) / d.vs;
    QTab q;
    memcpy(q.q, P.q[P.tq[c]], sizeof q.q);
    const long qo = pool_put(entries, pool, pool_cap, used, &q, sizeof q);
    const long dco = pool_put(entries, pool, pool_cap, used, &P.dct[c], sizeof(HuffTab));
    const long aco = pool_put(entries, pool, pool_cap, used, &P.act[c], sizeof(HuffTab));
    if (qo < 0 || dco < 0 || aco < 0) return false;
    d.qtab[c] = (int)qo;
    d.dctab[c] = (int)dco;
    d.actab[c] = (int)aco;
  }
  d.nblocks = off;
  d.coef_off = coef_off;
  return true;
}

struct HostSrc {
  const unsigned char* d;
  int byte(long long p) const { return d[p]; }
};

struct HostSink {
  short* coef;
  const JpegDesc* d;
  short* operator()(int c, int by, int bx) {
    short* b = coef + (d->coef_off + d->comp_off[c] + (long long)by * d->bw[c] + bx) * 64;
    memset(b, 0, 64 * sizeof(short));
    return b;
  }
};

// the entropy stage of one image without window or staging: bytes straight from `data`, blocks straight into `coef` -> status word
inline int entropy_flat(const unsigned char* data, const JpegDesc& d, const unsigned char* pool, short* coef) {
  std::vector<HuffTab> tabs(6);
  for (int k = 0; k < 6; ++k) memcpy(&tabs[k], pool + (k < 3 ? d.dctab[k] : d.actab[k - 3]), sizeof(HuffTab));
  HostSrc src{data};
  HostSink sink{coef, &d};
  BitState st = {0ull, 0, 0, 0, 0, d.scan_begin};
  int pred[3] = {0, 0, 0}, rst = 0;
  const long long total = (long long)d.mcux * d.mcuy;
  for (long long m = 0; m < total && !st.err; ++m) decode_mcu(d, tabs.data(), h_zz, st, src, pred, m, rst, sink);
  if (!st.err) end_interval(st, src, d.scan_end, rst, true);
  return st.err;
}

// the entropy stage of one image through entropy_windowed<WaveSim>; the wave's own memory is heap blocks of exactly the kernel's sizes
inline int entropy_windowed_host(const unsigned char* data, const JpegDesc& d, const unsigned char* pool, short* coef) {
  unsigned char* win = (unsigned char*)aligned_alloc(16, EWIN);
  short* stage = (short*)aligned_alloc(16, ESTAGE * 64 * sizeof(short));
  HuffTab* tabs = (HuffTab*)aligned_alloc(16, 6 * sizeof(HuffTab));
  long long* dest = (long long*)aligned_alloc(16, ESTAGE * sizeof(long long));
  unsigned char* zz = (unsigned char*)aligned_alloc(16, 64);
  EntropyShared* sh = (EntropyShared*)malloc(sizeof(EntropyShared));
  int pred[3];
  const int err = entropy_windowed<WaveSim>(data, &d, pool, coef, win, stage, tabs, dest, zz, h_zz, sh, pred);
  free(sh);
  free(zz);
  free(dest);
  free(tabs);
  free(stage);
  free(win);
  return err;
}

// launches 2 and 3 on the host: dequantise + IDCT of every block, then upsampling + colour conversion of every pixel
inline void idct_color_host(const JpegDesc& d, const unsigned char* pool, const short* coef, unsigned char* planes, unsigned char* out) {
  for (int b = 0; b < d.nblocks; ++b) {
    const int comp = b >= d.comp_off[2] ? 2 : b >= d.comp_off[1] ? 1 : 0;
    const long long gb = d.coef_off + b;
    int ws[64];
    for (int c = 0; c < 8; ++c) idct_col(coef + gb * 64, (const uint16_t*)(pool + d.qtab[comp]), c, ws);
    for (int r = 0; r < 8; ++r) idct_row(ws + r * 8, planes + gb * 64 + r * 8);
  }
  for (int y = 0; y < d.height; ++y)
    for (int x = 0; x < d.width; ++x) jpeg_pixel(planes + d.coef_off * 64, d, y, x, out + d.out_off + ((long long)y * d.width + x) * 3);
}

}  // namespace jpegcore
