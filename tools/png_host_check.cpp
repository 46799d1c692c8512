// Stand-alone memory check of the PNG routines (csrc/png_core.h: the code the GPU kernels and their host twin share), for a CPU build
// under AddressSanitizer + UndefinedBehaviorSanitizer.  No HIP, no Python:
//
//   python tools/gen_png_golden.py --dump /tmp/png_fixtures
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lite-mkd_amd/csrc tools/png_host_check.cpp -o /tmp/png_host_check
//   /tmp/png_host_check 4000 /tmp/png_fixtures/*.png
//
// Every file given is decoded as it is (a supported file must decode with status 0), then N times with seeded damage: one byte of the
// deflate stream altered, several bytes altered, the stream cut short, or a byte anywhere in the file altered (which the chunk walk
// has to survive).  Each case runs twice: through the flat host twin (decode_image_host) and through the inflate launch's own program
// (inflate_windowed: the 8 KiB window with its refill, the 32 KiB ring, the wave-wide copies and flushes) with the 64 lanes run in
// turn; the two must agree in status and scanline bytes.  All buffers are heap blocks of exactly the size the plan computes or the
// kernel declares, so a read or write past them is reported.  The program prints the count of each status word and exits non-zero
// if an undamaged supported file fails or the two disagree.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>

#include "png_core.h"

using namespace pngcore;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static long g_mismatch = 0;               // cases in which the windowed inflate and the flat one disagree
static unsigned rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (unsigned)(g_state >> 32);
}

// -> -1 unsupported, -2 malformed (both with `reason`), else the status word
static int run(const uint8_t* file, long long n, bool damage_stream, int mode, int& reason) {
  uint8_t* d = (uint8_t*)malloc((size_t)(n > 0 ? n : 1));
  memcpy(d, file, (size_t)n);
  Parsed P;
  int verdict = parse_png(d, n, P, reason);
  int result;
  if (verdict != PST_OK) {
    result = verdict == PST_UNSUPPORTED ? -1 : -2;
  } else {
    long long end = P.stream_end;
    if (damage_stream) {
      const long long len = P.stream_end - P.stream_begin;
      if (len > 0) {
        if (mode == 0) {
          d[P.stream_begin + rnd() % len] ^= (uint8_t)(1 + rnd() % 255);
        } else if (mode == 1) {
          for (int k = 0; k < 4; ++k) d[P.stream_begin + rnd() % len] = (uint8_t)rnd();
        } else {
          end = P.stream_begin + rnd() % len;
        }
      }
    }
    const long long total = (long long)P.H * (P.stride + 1);
    uint8_t* scratch = (uint8_t*)malloc((size_t)total);
    uint8_t* rows = (uint8_t*)malloc((size_t)(2 * P.stride));
    uint8_t* out = (uint8_t*)malloc((size_t)((long long)P.H * P.W * 3));
    uint8_t* stream = (uint8_t*)malloc((size_t)(end > 0 ? end : 1));      // the file up to the end of the stream: nothing beyond is readable
    memcpy(stream, d, (size_t)end);
    result = decode_image_host(stream, P.stream_begin, end, P.W, P.H, P.ctype, P.bpp, P.stride, P.pal, scratch, rows, out);
    // the inflate launch's own program (window refill, ring, wave-wide copies and flushes) with the 64 lanes run in turn: the same
    // status, and where the stream inflates, the same scanline bytes
    uint8_t* ring = (uint8_t*)malloc(RING);
    uint8_t* win = (uint8_t*)malloc(PWIN);
    uint8_t* scr2 = (uint8_t*)malloc((size_t)total);
    Huff* lit = (Huff*)malloc(sizeof(Huff));
    Huff* dst = (Huff*)malloc(sizeof(Huff));
    uint8_t* lens = (uint8_t*)malloc(320);
    int err = 0;
    unsigned trailer = 0;
    inflate_windowed<WaveSim>(stream, P.stream_begin, end, total, scr2, ring, win, *lit, *dst, lens, err, trailer);
    const bool inflated = result == PE_OK || result == PE_FILTER || result == PE_ADLER;
    if (inflated ? (err != PE_OK || memcmp(scratch, scr2, (size_t)total) != 0) : err != result) {
      fprintf(stderr, "the windowed inflate gives status %d, the flat one %d%s\n", err, result, inflated && err == PE_OK ? " (bytes differ)" : "");
      ++g_mismatch;
    }
    free(lens);
    free(dst);
    free(lit);
    free(scr2);
    free(win);
    free(ring);
    free(stream);
    free(out);
    free(rows);
    free(scratch);
  }
  free(d);
  return result;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s CASES file.png ...\n", argv[0]);
    return 2;
  }
  const int cases = atoi(argv[1]);
  std::map<int, long> hist;
  int failed = 0;
  long total_cases = 0;
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(f);
    int reason = 0;
    const int clean = run(file.data(), (long long)file.size(), false, 0, reason);
    if (clean == -2 || clean > 0) {
      fprintf(stderr, "%s: undamaged file fails: %s\n", argv[a], clean == -2 ? reason_text(reason) : "status word");
      ++failed;
    }
    // the large files take a share of the cases in proportion to nothing: every file gets the same count, capped for the big ones
    const int n = file.size() > 20000 ? cases / 20 + 1 : cases;
    for (int k = 0; k < n; ++k, ++total_cases) {
      const int mode = k % 4;
      int r;
      if (mode == 3) {
        std::vector<uint8_t> g(file);
        g[rnd() % g.size()] ^= (uint8_t)(1 + rnd() % 255);
        if (k % 8 == 7) g.resize(rnd() % g.size());
        r = run(g.data(), (long long)g.size(), false, 0, reason);
      } else {
        r = run(file.data(), (long long)file.size(), true, mode, reason);
      }
      hist[r]++;
    }
  }
  printf("%d files, %ld damaged cases; results (-2 malformed, -1 unsupported, 0 decoded, else status word):\n", argc - 2, total_cases);
  for (auto& kv : hist) printf("  %3d: %ld\n", kv.first, kv.second);
  if (g_mismatch) fprintf(stderr, "%ld cases in which the windowed and the flat inflate disagree\n", g_mismatch);
  return failed || g_mismatch ? 1 : 0;
}
