// Stand-alone memory check of the JPEG routines (csrc/jpeg_core.h: the code the GPU kernels and their host twins share), for a CPU build
// under AddressSanitizer + UndefinedBehaviorSanitizer.  No HIP, no Python:
//
//   python tools/gen_jpeg_golden.py --dump /tmp/jpeg_fixtures
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I lite-mkd_amd/csrc tools/jpeg_host_check.cpp -o /tmp/jpeg_host_check
//   /tmp/jpeg_host_check 3000 /tmp/jpeg_fixtures/*.jpg [--asis /tmp/jpeg_matrix/*.jpg]
//
// Every file given is decoded as it is (a supported file must decode with status 0), then N times with seeded damage: one byte of the
// scan altered, four bytes of the scan altered, the scan cut (with and without an EOI appended), one byte anywhere in the file altered,
// or a marker FF xx planted.  The files after --asis are decoded once, exactly as given (python tests/_jpeg_util.py DIR writes the
// tests' own corruption matrix there: the streams the GPU test sends are among them).  Each case runs twice: through the flat routines
// (entropy_flat: bytes straight from the file, blocks straight into coef) and through the entropy launch's own program
// (entropy_windowed: the 8 KiB window with its refill rule, the 48-block staging area and its flush) with the 64 lanes run in turn; the
// two must agree in verdict and status, and where the status is 0 in every coefficient.  All buffers are heap blocks of exactly the
// size the plan computes or the kernel declares (the file, the descriptor, the used prefix of the table pool, coef, planes, out, the
// window, the staging area), so a read or write past them is reported.  The program prints the count of each result and exits
// non-zero if an undamaged supported file fails or the two disagree.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>

#include "jpeg_core.h"

using namespace jpegcore;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static long g_mismatch = 0;               // cases in which the windowed program and the flat one disagree
static long g_windowed = 0;               // cases that reached the windowed program
static long g_refills = 0;                // of those, scans longer than one window
static unsigned rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (unsigned)(g_state >> 32);
}

// -> -1 unsupported, -2 malformed (both with `reason`), else the status word
static int run(const uint8_t* file, long long n, int& reason) {
  uint8_t* d = (uint8_t*)malloc((size_t)(n > 0 ? n : 1));      // the exact size (malloc aligns it to 16 bytes; the device copy needs 4)
  memcpy(d, file, (size_t)n);
  Parsed* P = new Parsed();
  const int verdict = parse_jpeg(d, n, *P, reason);
  int result;
  if (verdict != JST_OK) {
    result = verdict == JST_UNSUPPORTED ? -1 : -2;
  } else {
    JpegDesc* desc = (JpegDesc*)malloc(sizeof(JpegDesc));
    const long cap = pool_bytes(1);
    uint8_t* pool_all = (uint8_t*)malloc((size_t)cap);
    PoolEntries entries;
    long used = 0;
    if (!plan_image(*P, 0, 0, 0, *desc, entries, pool_all, cap, used)) {
      fprintf(stderr, "the pool of one image is too small\n");
      exit(1);
    }
    uint8_t* pool = (uint8_t*)aligned_alloc(16, (size_t)used);             // the used prefix, as uploaded
    memcpy(pool, pool_all, (size_t)used);
    free(pool_all);
    const size_t nb = (size_t)desc->nblocks;
    short* coef = (short*)aligned_alloc(16, nb * 64 * sizeof(short));
    short* coef2 = (short*)aligned_alloc(16, nb * 64 * sizeof(short));
    memset(coef, 0, nb * 64 * sizeof(short));
    memset(coef2, 0, nb * 64 * sizeof(short));
    uint8_t* planes = (uint8_t*)malloc(nb * 64);
    uint8_t* out = (uint8_t*)malloc((size_t)desc->width * desc->height * 3);
    result = entropy_flat(d, *desc, pool, coef);
    idct_color_host(*desc, pool, coef, planes, out);
    const int err = entropy_windowed_host(d, *desc, pool, coef2);
    ++g_windowed;
    if (desc->scan_end + 2 - (desc->scan_begin & ~3LL) > EWIN) ++g_refills;
    if (err != result || (err == 0 && memcmp(coef, coef2, nb * 64 * sizeof(short)) != 0)) {
      fprintf(stderr, "the windowed program gives status %d, the flat one %d%s\n", err, result, err == result ? " (coefficients differ)" : "");
      ++g_mismatch;
    }
    free(out);
    free(planes);
    free(coef2);
    free(coef);
    free(pool);
    free(desc);
  }
  delete P;
  free(d);
  return result;
}

static bool read_file(const char* path, std::vector<uint8_t>& file) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return false;
  }
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + got);
  fclose(f);
  return true;
}

static void print_hist(const char* title, long files, long cases, const std::map<int, long>& hist) {
  printf("%ld files, %ld %s; results (-2 malformed, -1 unsupported, 0 decoded, else status word):\n", files, cases, title);
  for (auto& kv : hist) printf("  %3d: %ld\n", kv.first, kv.second);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s CASES file.jpg ... [--asis file.jpg ...]\n", argv[0]);
    return 2;
  }
  const int cases = atoi(argv[1]);
  std::map<int, long> hist, hist_asis;
  int failed = 0;
  long total_cases = 0, files = 0, asis_files = 0;
  bool asis = false;
  for (int a = 2; a < argc; ++a) {
    if (strcmp(argv[a], "--asis") == 0) {
      asis = true;
      continue;
    }
    std::vector<uint8_t> file;
    if (!read_file(argv[a], file)) return 2;
    int reason = 0;
    const int clean = run(file.data(), (long long)file.size(), reason);
    if (asis) {
      hist_asis[clean]++;
      ++asis_files;
      continue;
    }
    ++files;
    if (clean == -2 || clean > 0) {
      fprintf(stderr, "%s: undamaged file fails: %s\n", argv[a], clean == -2 ? reason_text(reason) : "status word");
      ++failed;
    }
    // the scan of the undamaged file: [sb, se) with the end marker at se; a file without one (unsupported) takes whole-file damage only
    Parsed* P = new Parsed();
    const bool has_scan = parse_jpeg(file.data(), (long long)file.size(), *P, reason) == JST_OK && P->scan_end > P->scan_begin;
    const long long sb = P->scan_begin, len = P->scan_end - P->scan_begin;
    delete P;
    for (int k = 0; k < cases; ++k, ++total_cases) {
      std::vector<uint8_t> g(file);
      const int mode = has_scan ? k % 6 : 4 + k % 2;
      if (mode == 0) {
        g[sb + rnd() % len] ^= (uint8_t)(1 + rnd() % 255);
      } else if (mode == 1) {
        for (int j = 0; j < 4; ++j) g[sb + rnd() % len] = (uint8_t)rnd();
      } else if (mode == 2) {
        g.resize((size_t)(sb + rnd() % len));
      } else if (mode == 3) {
        g.resize((size_t)(sb + rnd() % len));
        g.push_back(0xFF);
        g.push_back(0xD9);
      } else if (mode == 4) {
        g[rnd() % g.size()] ^= (uint8_t)(1 + rnd() % 255);
      } else {
        const size_t at = (has_scan && (k / 6) % 2 == 0) ? (size_t)(sb + rnd() % len) : 2 + rnd() % (g.size() - 3);
        g[at] = 0xFF;
        if (at + 1 < g.size()) g[at + 1] = (uint8_t)rnd();
      }
      hist[run(g.data(), (long long)g.size(), reason)]++;
    }
  }
  print_hist("damaged cases", files, total_cases, hist);
  if (asis_files) print_hist("cases as given", asis_files, asis_files, hist_asis);
  printf("%ld cases ran the windowed program, %ld of them over a scan longer than one window; %ld disagree with the flat routines\n",
         g_windowed, g_refills, g_mismatch);
  return failed || g_mismatch ? 1 : 0;
}
