// PNG decoding routines shared by the GPU kernels and their host twin (csrc/png.hip).  This header also compiles as plain
// C++ (tools/png_host_check.cpp builds it without HIP): the qualifiers sit behind PNG_HD.
//
// Everything a file holds is outside input.  The routines here never index memory with a value read from the stream: compressed bytes
// come through a source object that clamps (Src::byte), output goes through a sink that the caller bounds (Out::put), table indices are
// bounded by construction, and every loop either consumes input or produces output, both of which are finite.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef PNG_HD
#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif
#endif
// the decoder's inner routines: always inlined, so that its state never passes through memory (see PNG_UNIFORM)
#define PNG_HDI PNG_HD __attribute__((always_inline))

// On the GPU the whole wave runs the decoder with identical values in every lane (csrc/png.hip): marking what comes out of memory as
// wave-uniform lets the compiler keep the decoder's state in scalar registers and run it on the scalar unit.  It never changes a value.
// (What a called function returns counts as lane-dependent too: build_huff's result is marked where it is used.)
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_UNIFORM(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define PNG_UNIFORM(x) ((int)(x))
#endif

namespace pngcore {

// status words of an image (0 = decoded)
enum {
  PE_OK = 0,
  PE_BLOCK_TYPE = 1,        // deflate block type 3
  PE_STORED_LEN = 2,        // stored block: LEN != ~NLEN
  PE_CODE_LENGTHS = 3,      // over-subscribed / incomplete code set, bad repeat, too many symbols, no end-of-block code
  PE_SYMBOL = 4,            // invalid literal / length or distance symbol
  PE_DISTANCE = 5,          // distance reaches before the first byte produced
  PE_TOO_MUCH = 6,          // more data than the image holds
  PE_ENDS_EARLY = 7,        // the stream (or the data it inflates to) ends before the image is complete
  PE_FILTER = 8,            // row filter type > 4
  PE_ADLER = 9,             // Adler-32 of the inflated bytes differs from the stream's trailer
  PE_WINDOW = 10,           // the decoder's LDS window was left (a defect of the decoder, never of the file)
};

constexpr int PLOOK = 9;                  // bits of the first-level lookup
constexpr int MAX_SYMS = 288;

// one canonical Huffman code: lookup of the first PLOOK bits (stream bit order), and count[] / sym[] for the longer codes
struct Huff {
  uint16_t look[1 << PLOOK];              // (code length << 9) | symbol, 0 = a longer (or no) code
  uint16_t count[16];                     // codes of each length
  uint16_t sym[MAX_SYMS];                 // symbols ordered by code
};

enum { HK_CODES = 0, HK_LENS = 1, HK_DISTS = 2 };

// zlib's inflate_table acceptance: an over-subscribed set is an error; an incomplete one too, unless it is a single code of length 1
// (and never for the code-length code); no code at all is accepted (every use of it is then an invalid symbol).  n <= MAX_SYMS.
PNG_HD int build_huff(Huff& h, const uint8_t* lens, int n, int kind) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int i = 0; i < n; ++i) h.count[PNG_UNIFORM(lens[i]) & 15]++;
  for (int i = 0; i < (1 << PLOOK); ++i) h.look[i] = 0;
  int max = 15;
  while (max > 0 && PNG_UNIFORM(h.count[max]) == 0) --max;
  h.count[0] = 0;
  if (max == 0) return kind == HK_CODES ? PE_CODE_LENGTHS : PE_OK;
  int left = 1;
  for (int l = 1; l < 16; ++l) {
    left <<= 1;
    left -= PNG_UNIFORM(h.count[l]);
    if (left < 0) return PE_CODE_LENGTHS;
  }
  if (left > 0 && (kind == HK_CODES || max != 1)) return PE_CODE_LENGTHS;
  int offs[16];
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + PNG_UNIFORM(h.count[l]);
  for (int i = 0; i < n; ++i) {
    const int l = PNG_UNIFORM(lens[i]) & 15;
    if (l) h.sym[offs[l]++] = (uint16_t)i;
  }
  unsigned code = 0;
  int idx = 0;
  for (int l = 1; l <= PLOOK; ++l) {
    const int cnt = PNG_UNIFORM(h.count[l]);
    for (int k = 0; k < cnt; ++k, ++code, ++idx) {
      unsigned rev = 0;
      for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
      for (unsigned j = rev; j < (1u << PLOOK); j += 1u << l) h.look[j] = (uint16_t)((l << 9) | h.sym[idx]);
    }
    code <<= 1;
  }
  return PE_OK;
}

// LSB-first bit reader.  Past the end of the stream it appends zero bits and counts them in `pad`: consuming one of them is the
// "ends early" error, found by the caller after each symbol (nbits < pad).
struct Bits {
  unsigned long long acc;                 // the low nbits bits are unconsumed
  int nbits, pad;
  long long pos;                          // next byte of the stream
};

template <class Src>
PNG_HDI void fill(Bits& s, const Src& src, long long end) {
  while (s.nbits <= 56) {
    unsigned b = 0;
    if (s.pos < end) b = (unsigned)src.byte(s.pos++) & 255u;
    else s.pad += 8;
    s.acc |= (unsigned long long)b << s.nbits;
    s.nbits += 8;
  }
}
PNG_HDI unsigned take(Bits& s, int n) {   // n <= 16, after fill
  const unsigned v = (unsigned)(s.acc & ((1ull << n) - 1));
  s.acc >>= n;
  s.nbits -= n;
  return v;
}

// needs 15 bits in the accumulator; -1 = no such code
PNG_HDI int huff_decode(Bits& s, const Huff& h) {
  const int e = PNG_UNIFORM(h.look[s.acc & ((1u << PLOOK) - 1)]);
  if (e) {
    take(s, e >> 9);
    return e & 511;
  }
  int code = 0, first = 0, index = 0;
  unsigned long long b = s.acc;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)(b & 1);
    b >>= 1;
    const int cnt = PNG_UNIFORM(h.count[len]);
    if (code - cnt < first) {
      take(s, len);
      return PNG_UNIFORM(h.sym[index + (code - first)]);
    }
    index += cnt;
    first += cnt;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

enum { ST_HEAD = 0, ST_STORED = 1, ST_CODES = 2, ST_TRAILER = 3, ST_DONE = 4 };
enum { OP_NONE = 0, OP_MATCH = 1, OP_STORED = 2, OP_DONE = 3, OP_ERR = 4 };
constexpr int STORED_CHUNK = 2048;        // bytes of a stored block handed to the caller at a time

struct Infl {
  Bits b;
  int state, last, stored_left, err;
  long long produced;                     // bytes of output so far
  unsigned trailer;                       // the stream's Adler-32 (valid in ST_DONE)
};
// what the caller has to do: MATCH = copy len bytes from `at - dist` to `at` (overlapping when dist < len);
// STORED = copy len bytes from stream position `src` to `at`
struct Op {
  int len, dist;
  long long src, at;
};

PNG_HDI void infl_init(Infl& s, long long begin) {
  s.b.acc = 0;
  s.b.nbits = s.b.pad = 0;
  s.b.pos = begin;
  s.state = ST_HEAD;
  s.last = s.stored_left = s.err = 0;
  s.produced = 0;
  s.trailer = 0;
}

PNG_HDI int infl_fail(Infl& s, int e) {
  s.err = e;
  return OP_ERR;
}

// the block header; for a dynamic block the two code sets (lens: 320 bytes of scratch)
template <class Src>
PNG_HDI int infl_head(Infl& s, Huff& lit, Huff& dst, uint8_t* lens, const Src& src, long long end) {
  fill(s.b, src, end);
  s.last = (int)take(s.b, 1);
  const int type = (int)take(s.b, 2);
  if (type == 3) return PE_BLOCK_TYPE;
  if (type == 0) {
    take(s.b, s.b.nbits & 7);             // to the byte boundary
    const unsigned len = take(s.b, 16), nlen = take(s.b, 16);
    if (s.b.nbits < s.b.pad) return PE_ENDS_EARLY;
    if (len != ((~nlen) & 0xFFFFu)) return PE_STORED_LEN;
    s.b.pos -= (s.b.nbits - s.b.pad) >> 3;      // hand back the whole bytes read ahead: the stored bytes are copied from the stream
    s.b.acc = 0;
    s.b.nbits = s.b.pad = 0;
    s.stored_left = (int)len;
    s.state = ST_STORED;
    return PE_OK;
  }
  if (type == 1) {
    for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    (void)PNG_UNIFORM(build_huff(lit, lens, 288, HK_LENS));
    for (int i = 0; i < 32; ++i) lens[i] = 5;   // symbols 30 and 31 take code space and are refused where they are used
    (void)PNG_UNIFORM(build_huff(dst, lens, 32, HK_DISTS));
    s.state = ST_CODES;
    return PE_OK;
  }
  const int nlen = (int)take(s.b, 5) + 257, ndist = (int)take(s.b, 5) + 1, ncode = (int)take(s.b, 4) + 4;
  if (nlen > 286 || ndist > 30) return PE_CODE_LENGTHS;
  const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = 0; i < 19; ++i) lens[i] = 0;
  for (int i = 0; i < ncode; ++i) {
    fill(s.b, src, end);
    lens[order[i]] = (uint8_t)take(s.b, 3);
  }
  if (s.b.nbits < s.b.pad) return PE_ENDS_EARLY;
  if (PNG_UNIFORM(build_huff(dst, lens, 19, HK_CODES))) return PE_CODE_LENGTHS;      // dst serves as the code-length code until it is rebuilt below
  const int total = nlen + ndist;
  int i = 0;
  while (i < total) {
    fill(s.b, src, end);
    const int sym = huff_decode(s.b, dst);
    if (sym < 0 || sym > 18) return PE_CODE_LENGTHS;
    if (sym < 16) {
      lens[i++] = (uint8_t)sym;
    } else {
      int rep, val = 0;
      if (sym == 16) {
        if (i == 0) return PE_CODE_LENGTHS;
        val = PNG_UNIFORM(lens[i - 1]);
        rep = 3 + (int)take(s.b, 2);
      } else if (sym == 17) {
        rep = 3 + (int)take(s.b, 3);
      } else {
        rep = 11 + (int)take(s.b, 7);
      }
      if (i + rep > total) return PE_CODE_LENGTHS;
      while (rep--) lens[i++] = (uint8_t)val;
    }
    if (s.b.nbits < s.b.pad) return PE_ENDS_EARLY;
  }
  if (PNG_UNIFORM(lens[256]) == 0) return PE_CODE_LENGTHS;
  if (PNG_UNIFORM(build_huff(lit, lens, nlen, HK_LENS))) return PE_CODE_LENGTHS;
  if (PNG_UNIFORM(build_huff(dst, lens + nlen, ndist, HK_DISTS))) return PE_CODE_LENGTHS;
  s.state = ST_CODES;
  return PE_OK;
}

// Decode until the caller has something to do (-> OP_MATCH / OP_STORED with `op` filled; the state has already moved past it), the
// stream is complete (OP_DONE), an error stops the image (OP_ERR, s.err) or a limit is reached (OP_NONE): the next stream byte lies
// beyond pos_limit, or out_limit bytes have been produced.  Literals go to out.put(position, byte).  `total` bounds the output:
// nothing is put or handed over at or beyond it.
template <class Src, class Out>
PNG_HDI int inflate_step(Infl& s, Huff& lit, Huff& dst, uint8_t* lens, const Src& src, long long end, long long total, long long pos_limit,
                        long long out_limit, Out& out, Op& op) {
  for (;;) {
    if (s.state == ST_DONE) return OP_DONE;
    if (s.b.pos > pos_limit || s.produced >= out_limit) return OP_NONE;
    if (s.state == ST_HEAD) {
      const int e = infl_head(s, lit, dst, lens, src, end);
      if (e) return infl_fail(s, e);
    } else if (s.state == ST_STORED) {
      if (s.stored_left == 0) {
        s.state = s.last ? ST_TRAILER : ST_HEAD;
        continue;
      }
      long long n = s.stored_left < STORED_CHUNK ? s.stored_left : STORED_CHUNK;
      if (s.b.pos + n > end) n = end - s.b.pos;
      if (n <= 0) return infl_fail(s, PE_ENDS_EARLY);
      if (s.produced + n > total) return infl_fail(s, PE_TOO_MUCH);
      op.len = (int)n;
      op.dist = 0;
      op.src = s.b.pos;
      op.at = s.produced;
      s.b.pos += n;
      s.produced += n;
      s.stored_left -= (int)n;
      return OP_STORED;
    } else if (s.state == ST_CODES) {
      fill(s.b, src, end);
      int sym = huff_decode(s.b, lit);
      if (sym < 0) return infl_fail(s, PE_SYMBOL);
      if (s.b.nbits < s.b.pad) return infl_fail(s, PE_ENDS_EARLY);
      if (sym < 256) {
        if (s.produced >= total) return infl_fail(s, PE_TOO_MUCH);
        out.put(s.produced++, (uint8_t)sym);
        continue;
      }
      if (sym == 256) {
        s.state = s.last ? ST_TRAILER : ST_HEAD;
        continue;
      }
      sym -= 257;
      if (sym >= 29) return infl_fail(s, PE_SYMBOL);
      int len;
      if (sym < 8) len = 3 + sym;
      else if (sym == 28) len = 258;
      else {
        const int extra = (sym - 4) >> 2;
        len = 3 + ((4 + (sym & 3)) << extra) + (int)take(s.b, extra);
      }
      const int dsym = huff_decode(s.b, dst);         // 57 - 15 - 5 bits are left: enough for 15 + 13
      if (dsym < 0 || dsym >= 30) return infl_fail(s, PE_SYMBOL);
      int dist;
      if (dsym < 4) dist = 1 + dsym;
      else {
        const int extra = (dsym >> 1) - 1;
        dist = 1 + ((2 + (dsym & 1)) << extra) + (int)take(s.b, extra);
      }
      if (s.b.nbits < s.b.pad) return infl_fail(s, PE_ENDS_EARLY);
      if (dist > s.produced) return infl_fail(s, PE_DISTANCE);
      if (s.produced + len > total) return infl_fail(s, PE_TOO_MUCH);
      op.len = len;
      op.dist = dist;
      op.src = 0;
      op.at = s.produced;
      s.produced += len;
      return OP_MATCH;
    } else {      // ST_TRAILER
      take(s.b, s.b.nbits & 7);
      fill(s.b, src, end);
      if (s.b.nbits - s.b.pad < 32) return infl_fail(s, PE_ENDS_EARLY);
      const unsigned b0 = take(s.b, 8), b1 = take(s.b, 8), b2 = take(s.b, 8), b3 = take(s.b, 8);
      s.trailer = (b0 << 24) | (b1 << 16) | (b2 << 8) | b3;
      if (s.produced != total) return infl_fail(s, PE_ENDS_EARLY);
      s.state = ST_DONE;
      return OP_DONE;
    }
  }
}

// ---- the inflate of one image by a wave (launch 1 of lmkd_png_decode): compressed bytes through a window, output through a ring ----
// The serial decoder (inflate_step) runs with the same values in every lane; what a wave does in parallel stands in loops over the
// lanes, for (t = Wv::first(); t < 64; t += Wv::STEP), and Wv::sync() separates the phases.  On the GPU a lane runs its own iteration
// and sync is the workgroup barrier; WaveSim runs the 64 lanes one after the other on one thread, which is the same program in plain
// C++ (tools/png_host_check.cpp runs it under the sanitizers with win, ring and scr as heap blocks of exactly these sizes).
constexpr int RING = 32768, RMASK = RING - 1;      // the deflate window
constexpr int PWIN = 8192;                // window of compressed bytes
constexpr int PGUARD = 1024;              // refill when fewer are left: a dynamic block header reads at most 17 + 57 + 320 x 14 bits
                                          // = 570 bytes, a symbol 6, + the accumulator's 8 bytes of lookahead
constexpr int PFLUSH = 16384;             // write the ring out when this much is unwritten: + one operation of at most
                                          // STORED_CHUNK bytes stays below RING, so unwritten bytes are never overwritten
static_assert(PFLUSH + STORED_CHUNK <= RING && PFLUSH + 258 <= RING, "ring");

struct WaveSim {
  enum { STEP = 1, HELD = 64 };           // HELD: lanes whose registers one thread has to keep between two phases
  static int first() { return 0; }
  static void sync() {}
};

struct WinSrc {
  const uint8_t* win;
  long long base;
  mutable int over;
  PNG_HDI int byte(long long p) const {
    const long long o = p - base;
    if (o < 0 || o >= PWIN) {
      over = 1;
      return 0;
    }
    return PNG_UNIFORM(win[o]);
  }
};
template <class Wv>
struct RingOut {
  uint8_t* ring;
  PNG_HDI void put(long long p, uint8_t v) {
    if (Wv::first() == 0) ring[p & RMASK] = v;
  }
};

// stream = data[sb, se) (data 4-byte aligned; the bytes from sb & ~3 on are readable), total = H * (stride + 1) bytes written to scr
// (4-byte aligned); ring: RING bytes, win: PWIN bytes, both 4-byte aligned.  -> err (a status word) and the stream's Adler-32 trailer
template <class Wv>
PNG_HDI void inflate_windowed(const uint8_t* data, long long sb, long long se, long long total, uint8_t* scr, uint8_t* ring, uint8_t* win,
                              Huff& lit, Huff& dst, uint8_t* lens, int& err, unsigned& trailer) {
  const long long lo = sb & ~3LL;
  // from here on every lane holds the same values: the decoder state, the window base, what has been written out
  Infl st;
  infl_init(st, sb);
  long long base = lo;                    // stream position of win[0], a multiple of 4
  bool refill = true;
  long long flushed = 0;                  // bytes written to the scratch so far, a multiple of 4
  for (;;) {
    if (refill) {
      Wv::sync();                         // (the window is not being read)
      long long n = se - base < PWIN ? se - base : PWIN;
      if (n < 0) n = 0;
      const uint8_t* g = data + base;
      const int nd = (int)(n >> 2);
      for (int t = Wv::first(); t < 64; t += Wv::STEP) {
        for (int i = t; i < nd; i += 64) ((uint32_t*)win)[i] = ((const uint32_t*)g)[i];
        for (int i = nd * 4 + t; i < n; i += 64) win[i] = g[i];
      }
      Wv::sync();
    }
    WinSrc src{win, base, 0};
    RingOut<Wv> out{ring};
    const bool covers_end = base + PWIN >= se;
    const long long pos_limit = covers_end ? ((long long)1 << 62) : base + PWIN - PGUARD;
    Op op = {0, 0, 0, 0};
    int kind = inflate_step(st, lit, dst, lens, src, se, total, pos_limit, flushed + PFLUSH, out, op);
    if (src.over && kind != OP_ERR) {
      st.err = PE_WINDOW;
      kind = OP_ERR;
    }
    refill = !covers_end && st.b.pos > pos_limit && kind != OP_ERR && kind != OP_DONE;
    if (refill) {                         // 8 bytes behind the reader: a stored block hands back the bytes it had read ahead
      const long long nb = (st.b.pos - 8) & ~3LL;
      base = nb < lo ? lo : nb;
    }
    Wv::sync();                           // lane 0's literals are in the ring
    if (kind == OP_MATCH) {                // len <= 258 <= 5 x 64: every source byte is read before any is written
      const int len = op.len, dist = op.dist;
      const long long at = op.at;
      uint8_t v[Wv::HELD][5];
      for (int t = Wv::first(); t < 64; t += Wv::STEP) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const int i = t + 64 * j;
          v[t % Wv::HELD][j] = 0;
          if (i < len) v[t % Wv::HELD][j] = ring[(at - dist + (dist >= len ? i : i % dist)) & RMASK];
        }
      }
      Wv::sync();
      for (int t = Wv::first(); t < 64; t += Wv::STEP) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const int i = t + 64 * j;
          if (i < len) ring[(at + i) & RMASK] = v[t % Wv::HELD][j];
        }
      }
    } else if (kind == OP_STORED) {
      const int len = op.len;
      const long long at = op.at, from = op.src;
      for (int t = Wv::first(); t < 64; t += Wv::STEP)
        for (int i = t; i < len; i += 64) {
          const long long p = from + i;
          ring[(at + i) & RMASK] = (p >= sb && p < se) ? data[p] : (uint8_t)0;
        }
    }
    Wv::sync();
    long long prod = st.produced;
    if (prod > total) prod = total;       // (inflate_step never passes total)
    if (kind == OP_DONE || prod - flushed >= PFLUSH) {
      const long long hi = kind == OP_DONE ? prod : (prod & ~3LL);
      const int nw = (int)((hi - flushed) >> 2);
      for (int t = Wv::first(); t < 64; t += Wv::STEP) {
        for (int i = t; i < nw; i += 64)
          ((uint32_t*)(scr + flushed))[i] = *(const uint32_t*)(ring + ((flushed + 4LL * i) & RMASK));
        for (long long p = flushed + 4LL * nw + t; p < hi; p += 64) scr[p] = ring[p & RMASK];
      }
      flushed = hi & ~3LL;
      Wv::sync();                         // the ring has been read before the decoder writes it again
    }
    if (kind == OP_DONE || kind == OP_ERR) break;
  }
  err = st.err;
  trailer = st.trailer;
}

// ---- Adler-32 over chunks: (A, B) after n more bytes with s1 = sum b_i and s2 = sum (n - i) b_i, both reduced mod 65521 ----
constexpr unsigned ADLER_MOD = 65521u;
PNG_HD void adler_combine(unsigned& A, unsigned& B, unsigned n, unsigned s1, unsigned s2) {
  B = (unsigned)(((unsigned long long)B + (unsigned long long)(n % ADLER_MOD) * A + s2) % ADLER_MOD);
  A = (A + s1) % ADLER_MOD;
}

// ---- row filters (PNG specification 9.2) ----
PNG_HD int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// Sub / Average / Paeth along a row for byte lane k of the pixel (the serial direction): raw = the filtered bytes after the filter
// byte, prev = the row above, already reconstructed (zeros above the first row)
PNG_HD void unfilter_lane(int ft, const uint8_t* raw, const uint8_t* prev, uint8_t* cur, int k, int bpp, int stride) {
  int a = 0, c = 0;
  for (int i = k; i < stride; i += bpp) {
    const int b = prev[i];
    const int pred = ft == 1 ? a : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
    a = (raw[i] + pred) & 255;
    cur[i] = (uint8_t)a;
    c = b;
  }
}

// one reconstructed pixel -> RGB as PIL's convert("RGB") gives it: gray replicated, palette looked up, alpha dropped
PNG_HD void expand_pixel(int ctype, const uint8_t* px, const uint8_t* pal, uint8_t* rgb) {
  if (ctype == 0) {
    rgb[0] = rgb[1] = rgb[2] = px[0];
  } else if (ctype == 3) {
    const uint8_t* e = pal + 3 * (int)px[0];
    rgb[0] = e[0];
    rgb[1] = e[1];
    rgb[2] = e[2];
  } else {
    rgb[0] = px[0];
    rgb[1] = px[1];
    rgb[2] = px[2];
  }
}

// ---- the whole image on one thread (the host twin; the kernels split the same steps over a wave) ----
struct FlatSrc {
  const uint8_t* d;
  int byte(long long p) const { return d[p]; }
};
struct FlatOut {
  uint8_t* o;
  void put(long long p, uint8_t v) { o[p] = v; }
};

// stream = data[begin, end) (after the zlib header); scratch: H * (stride + 1) bytes; rows: 2 * stride bytes; out: H * W * 3
inline int decode_image_host(const uint8_t* data, long long begin, long long end, int W, int H, int ctype, int bpp, int stride,
                             const uint8_t* pal, uint8_t* scratch, uint8_t* rows, uint8_t* out) {
  const long long total = (long long)H * (stride + 1);
  Infl s;
  infl_init(s, begin);
  Huff lit, dst;
  uint8_t lens[320];
  FlatSrc src{data};
  FlatOut sink{scratch};
  Op op;
  for (;;) {
    const int k = inflate_step(s, lit, dst, lens, src, end, total, (long long)1 << 62, (long long)1 << 62, sink, op);
    if (k == OP_ERR) return s.err;
    if (k == OP_DONE) break;
    if (k == OP_MATCH) {
      for (int i = 0; i < op.len; ++i) scratch[op.at + i] = scratch[op.at - op.dist + i];
    } else if (k == OP_STORED) {
      for (int i = 0; i < op.len; ++i) scratch[op.at + i] = data[op.src + i];
    }
  }
  unsigned A = 1, B = 0;
  uint8_t* prev = rows;
  uint8_t* cur = rows + stride;
  for (int i = 0; i < stride; ++i) prev[i] = 0;
  for (int y = 0; y < H; ++y) {
    const uint8_t* raw = scratch + (long long)y * (stride + 1);
    const unsigned n = (unsigned)stride + 1;
    unsigned long long s1 = 0, s2 = 0;
    for (unsigned i = 0; i < n; ++i) {
      s1 += raw[i];
      s2 += (unsigned long long)(n - i) * raw[i];
    }
    adler_combine(A, B, n, (unsigned)(s1 % ADLER_MOD), (unsigned)(s2 % ADLER_MOD));
    const int ft = raw[0];
    if (ft > 4) return PE_FILTER;
    if (ft == 0) {
      for (int i = 0; i < stride; ++i) cur[i] = raw[1 + i];
    } else if (ft == 2) {
      for (int i = 0; i < stride; ++i) cur[i] = (uint8_t)(raw[1 + i] + prev[i]);
    } else {
      for (int k = 0; k < bpp; ++k) unfilter_lane(ft, raw + 1, prev, cur, k, bpp, stride);
    }
    for (int x = 0; x < W; ++x) expand_pixel(ctype, cur + x * bpp, pal, out + ((long long)y * W + x) * 3);
    uint8_t* t = prev;
    prev = cur;
    cur = t;
  }
  if (((B << 16) | A) != s.trailer) return PE_ADLER;
  return PE_OK;
}

// ---- the container: chunk walk, IHDR, the zlib header (host only) ----
enum { PST_OK = 0, PST_UNSUPPORTED = 1, PST_MALFORMED = 2 };
enum {
  PR_NONE = 0,
  PR_INTERLACE = 1, PR_DEPTH = 2, PR_GRAY_ALPHA = 3, PR_APNG = 4, PR_SIZE = 5,
  PR_SIGNATURE = 20, PR_IHDR_FIRST = 21, PR_IHDR = 22, PR_TRUNCATED = 23, PR_CRC = 24, PR_NO_PLTE = 25, PR_NO_IDAT = 26, PR_ZLIB = 27,
  PR_PLTE = 28, PR_HUGE = 29,
};
constexpr int PNG_MAX_DIM = 4096;         // a larger image is left to PIL (unsupported), up to the limits below
// beyond these the header is taken for damage (malformed), so that no size it claims reaches the caller's buffer sizes; PIL refuses
// a file of that many pixels as a decompression bomb
constexpr unsigned PNG_SANE_DIM = 65535, PNG_SANE_PIXELS = 1u << 27;

inline const char* reason_text(int r) {
  switch (r) {
    case PR_NONE: return "supported";
    case PR_INTERLACE: return "Adam7 interlace";
    case PR_DEPTH: return "bit depth other than 8";
    case PR_GRAY_ALPHA: return "gray + alpha";
    case PR_APNG: return "APNG";
    case PR_SIZE: return "size above 4096";
    case PR_SIGNATURE: return "bad signature";
    case PR_IHDR_FIRST: return "IHDR is not the first chunk";
    case PR_IHDR: return "bad IHDR";
    case PR_TRUNCATED: return "truncated chunk";
    case PR_CRC: return "CRC mismatch";
    case PR_NO_PLTE: return "palette image without PLTE";
    case PR_NO_IDAT: return "no IDAT";
    case PR_ZLIB: return "bad zlib header";
    case PR_PLTE: return "bad PLTE";
    case PR_HUGE: return "size above 65535 or more than 2^27 pixels";
    default: return "unknown";
  }
}

struct CrcTable {                         // slicing by 8: t[k][b] = the CRC of byte b followed by k zero bytes
  unsigned t[8][256];
  CrcTable() {
    for (unsigned i = 0; i < 256; ++i) {
      unsigned c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][i] = c;
    }
    for (unsigned i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = t[0][t[k - 1][i] & 255] ^ (t[k - 1][i] >> 8);
  }
};

inline unsigned crc32_png(const uint8_t* p, long long n) {
  static const CrcTable table;            // (initialised once, also when several loader threads plan at the same time)
  unsigned c = 0xFFFFFFFFu;
  long long i = 0;
  for (; i + 8 <= n; i += 8) {
    const unsigned a = c ^ ((unsigned)p[i] | ((unsigned)p[i + 1] << 8) | ((unsigned)p[i + 2] << 16) | ((unsigned)p[i + 3] << 24));
    c = table.t[7][a & 255] ^ table.t[6][(a >> 8) & 255] ^ table.t[5][(a >> 16) & 255] ^ table.t[4][a >> 24] ^ table.t[3][p[i + 4]] ^
        table.t[2][p[i + 5]] ^ table.t[1][p[i + 6]] ^ table.t[0][p[i + 7]];
  }
  for (; i < n; ++i) c = table.t[0][(c ^ p[i]) & 255] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

struct Parsed {
  int W = 0, H = 0, depth = 0, ctype = 0, bpp = 0, stride = 0;
  int npal = 0;
  uint8_t pal[768];
  long long stream_begin = 0, stream_end = 0;   // the compacted zlib stream after its 2-byte header (relative to the image)
};

inline unsigned be32(const uint8_t* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

// -> verdict; for a supported image the IDAT payloads are moved together, in place, to where the first one begins (compact = true)
inline int parse_png(uint8_t* d, long long n, Parsed& P, int& reason, bool compact = true) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  reason = PR_NONE;
  if (n < 8) return reason = PR_SIGNATURE, PST_MALFORMED;
  for (int i = 0; i < 8; ++i)
    if (d[i] != sig[i]) return reason = PR_SIGNATURE, PST_MALFORMED;
  long long pos = 8;
  bool first = true, have_plte = false, have_iend = false, apng = false;
  int unsupported = PR_NONE;
  long long nidat = 0, idat_first = -1;
  for (int i = 0; i < 768; ++i) P.pal[i] = 0;
  // pass 1: structure and CRCs
  while (!have_iend) {
    if (pos + 12 > n) return reason = PR_TRUNCATED, PST_MALFORMED;
    const unsigned len = be32(d + pos);
    const uint8_t* ty = d + pos + 4;
    if (len > 0x7FFFFFFFu || pos + 12 + (long long)len > n) return reason = PR_TRUNCATED, PST_MALFORMED;
    const uint8_t* body = d + pos + 8;
    const bool is_ihdr = ty[0] == 'I' && ty[1] == 'H' && ty[2] == 'D' && ty[3] == 'R';
    const bool is_plte = ty[0] == 'P' && ty[1] == 'L' && ty[2] == 'T' && ty[3] == 'E';
    const bool is_idat = ty[0] == 'I' && ty[1] == 'D' && ty[2] == 'A' && ty[3] == 'T';
    const bool is_iend = ty[0] == 'I' && ty[1] == 'E' && ty[2] == 'N' && ty[3] == 'D';
    if (first != is_ihdr) return reason = PR_IHDR_FIRST, PST_MALFORMED;
    if (is_ihdr || is_plte || is_idat || is_iend)
      if (crc32_png(ty, 4 + (long long)len) != be32(body + len)) return reason = PR_CRC, PST_MALFORMED;
    if (is_ihdr) {
      if (len != 13) return reason = PR_IHDR, PST_MALFORMED;
      const unsigned w = be32(body), h = be32(body + 4);
      P.depth = body[8];
      P.ctype = body[9];
      if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || body[10] != 0 || body[11] != 0 || body[12] > 1)
        return reason = PR_IHDR, PST_MALFORMED;
      const int dp = P.depth, ct = P.ctype;
      const bool ok = (ct == 0 && (dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16)) || ((ct == 2 || ct == 4 || ct == 6) && (dp == 8 || dp == 16)) ||
                      (ct == 3 && (dp == 1 || dp == 2 || dp == 4 || dp == 8));
      if (!ok) return reason = PR_IHDR, PST_MALFORMED;
      if (w > PNG_SANE_DIM || h > PNG_SANE_DIM || (unsigned long long)w * h > PNG_SANE_PIXELS) return reason = PR_HUGE, PST_MALFORMED;
      if (body[12] == 1) unsupported = PR_INTERLACE;
      else if (dp != 8) unsupported = PR_DEPTH;
      else if (ct == 4) unsupported = PR_GRAY_ALPHA;
      else if (w > (unsigned)PNG_MAX_DIM || h > (unsigned)PNG_MAX_DIM) unsupported = PR_SIZE;
      P.W = (int)w;
      P.H = (int)h;
      first = false;
    } else if (is_plte) {
      if (len == 0 || len > 768 || len % 3 != 0) return reason = PR_PLTE, PST_MALFORMED;
      if (!have_plte && nidat == 0) {
        for (unsigned i = 0; i < len; ++i) P.pal[i] = body[i];
        P.npal = (int)(len / 3);
      }
      have_plte = true;
    } else if (is_idat) {
      if (nidat == 0) {
        if (P.ctype == 3 && !have_plte) return reason = PR_NO_PLTE, PST_MALFORMED;
        idat_first = pos;
      }
      ++nidat;
    } else if (is_iend) {
      have_iend = true;
    } else if (ty[0] == 'a' && ty[1] == 'c' && ty[2] == 'T' && ty[3] == 'L') {
      apng = true;
    }
    pos += 12 + (long long)len;
  }
  if (nidat == 0) return reason = PR_NO_IDAT, PST_MALFORMED;
  if (apng && !unsupported) unsupported = PR_APNG;
  // the zlib header = the first two bytes of the concatenated payloads
  uint8_t zh[2];
  int nz = 0;
  for (long long p = idat_first; nz < 2 && p + 12 <= n;) {
    const unsigned len = be32(d + p);
    const uint8_t* ty = d + p + 4;
    if (ty[0] == 'I' && ty[1] == 'D' && ty[2] == 'A' && ty[3] == 'T')
      for (unsigned i = 0; i < len && nz < 2; ++i) zh[nz++] = d[p + 8 + i];
    else if (ty[0] == 'I' && ty[1] == 'E' && ty[2] == 'N' && ty[3] == 'D')
      break;
    p += 12 + (long long)len;
  }
  if (nz < 2 || (zh[0] & 15) != 8 || (zh[0] >> 4) > 7 || (zh[1] & 0x20) || ((zh[0] << 8) | zh[1]) % 31 != 0) return reason = PR_ZLIB, PST_MALFORMED;
  if (unsupported) return reason = unsupported, PST_UNSUPPORTED;
  P.bpp = P.ctype == 0 || P.ctype == 3 ? 1 : P.ctype == 2 ? 3 : 4;
  P.stride = P.W * P.bpp;
  // pass 2: move the payloads together
  long long w = idat_first + 8;
  P.stream_begin = w + 2;
  for (long long p = idat_first; p + 12 <= n;) {
    const unsigned len = be32(d + p);
    const uint8_t ty0 = d[p + 4], ty1 = d[p + 5], ty2 = d[p + 6], ty3 = d[p + 7];
    const long long next = p + 12 + (long long)len;
    if (ty0 == 'I' && ty1 == 'D' && ty2 == 'A' && ty3 == 'T') {
      if (compact) {
        if (w != p + 8) memmove(d + w, d + p + 8, len);             // w <= p + 8: the range moves down
      }
      w += len;
    } else if (ty0 == 'I' && ty1 == 'E' && ty2 == 'N' && ty3 == 'D') {
      break;
    }
    p = next;
  }
  P.stream_end = w;
  return PST_OK;
}

}  // namespace pngcore
