// CPU sanitizer pass over the resampler's bank builder: built by tests/test_sanitize_resample_cpu.py as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/sanitize/resample_fuzz.cpp
// against lightning_asr_amd/csrc/resample.h - the SAME source liblasr.so compiles (resample.hip wraps it).  No GPU, no HIP.
// Exit code 0 = every case behaved (a clean error or a consistent image); any sanitizer report aborts with a non-zero code.
//
//   1. known answers: geometry of the conversions the product uses, per-phase tap sums (DC gain) within 1.0000 .. 1.0009, the image
//      header's offsets and tiling inside the limits the kernel relies on;
//   2. hostile arguments - zero / negative / huge rates, factors above 1024, tap counts above 2^20, rolloff 0 / NaN / inf /
//      denormal / above 1, lpw outside [1, 64], more than 8 conversions, null lists, short destinations - each a clean error;
//   3. 1 000 LCG-driven (rates, lpw, rolloff) draws: each either refused, or an image written into an EXACTLY sized heap block
//      (ASan guards both ends) whose header is consistent;
//   4. out_len against the rational definition, overflow included.
#include "../../lightning_asr_amd/csrc/resample.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace lasr::resample;

static int g_fail = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

static uint64_t g_lcg = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_lcg >> 33); }

// what the kernel relies on before it reads an image
static void check_image(const std::vector<char>& img, int n_conv, const char* what) {
  CHECK(img.size() >= (size_t)kHeaderWords * 4, "%s: image smaller than its header", what);
  if (img.size() < (size_t)kHeaderWords * 4) return;
  int32_t head[kHeaderWords];
  memcpy(head, img.data(), sizeof(head));
  CHECK((uint32_t)head[0] == kMagic && head[1] == n_conv, "%s: magic / count", what);
  const int64_t words = (int64_t)(img.size() / 4);
  int64_t expect = kHeaderWords;
  for (int i = 0; i < n_conv; ++i) {
    Conv c;
    memcpy(&c, head + 16 + 8 * i, sizeof(c));
    CHECK(c.up >= 1 && c.up <= kMaxFactor && c.down >= 1 && c.down <= kMaxFactor, "%s: factors", what);
    CHECK(gcd64(c.up, c.down) == 1, "%s: factors not reduced", what);
    CHECK(c.nblk >= 1 && (int64_t)c.nblk * c.up <= kMaxTile, "%s: tile %d x %d", what, c.nblk, c.up);
    if (c.up == 1 && c.down == 1) { CHECK(c.taps == 0, "%s: identity with taps", what); continue; }
    CHECK(c.taps == 2 * c.width + c.down && c.width >= 1, "%s: taps", what);
    CHECK((int64_t)c.up * c.taps <= kMaxBankWords, "%s: bank too large", what);
    CHECK(c.offset == expect && (int64_t)c.offset + (int64_t)c.up * c.taps <= words, "%s: taps outside the image", what);
    CHECK(c.kc >= 1 && c.kc <= kMaxChunk && c.kc <= c.taps, "%s: chunk", what);
    CHECK((int64_t)(c.nblk - 1) * c.down + c.kc <= kSpanCap, "%s: staged span %d x %d + %d", what, c.nblk, c.down, c.kc);
    expect += (int64_t)c.up * c.taps;
  }
  CHECK(expect == words, "%s: image size", what);
}

static bool build(const int32_t* a, const int32_t* b, int n, int lpw, double rolloff, std::vector<char>* img, std::string* err) {
  const size_t bytes = bank_bytes(a, b, n, lpw, rolloff, err);
  if (!bytes) return false;
  img->assign(bytes, (char)0x5a);
  const int rc = bank_write(a, b, n, lpw, rolloff, img->data(), bytes, err);
  CHECK(rc == kOk, "bank_bytes accepted what bank_write refused: %s", err->c_str());
  return rc == kOk;
}

static void expect_error(const int32_t* a, const int32_t* b, int n, int lpw, double rolloff, const char* what) {
  std::string err;
  CHECK(bank_bytes(a, b, n, lpw, rolloff, &err) == 0 && !err.empty(), "%s: bank_bytes accepted it", what);
  char small[8];
  err.clear();
  CHECK(bank_write(a, b, n, lpw, rolloff, small, sizeof(small), &err) == kErrArg && !err.empty(), "%s: bank_write accepted it", what);
}

int main() {
  // ---- 1. known answers
  struct Known { int32_t in, out, up, down, width, taps; };
  const Known known[] = {{44100, 16000, 160, 441, 17, 475}, {48000, 16000, 1, 3, 19, 41}, {8000, 16000, 2, 1, 7, 15},
                         {9, 10, 10, 9, 7, 23},             {11, 10, 10, 11, 7, 25},      {16000, 16000, 1, 1, 0, 0}};
  for (const Known& k : known) {
    Conv c;
    std::string err;
    CHECK(plan(k.in, k.out, 6, 0.99, &c, &err) == kOk, "%d -> %d refused: %s", k.in, k.out, err.c_str());
    CHECK(c.up == k.up && c.down == k.down && c.width == k.width && c.taps == k.taps, "%d -> %d: geometry %d/%d width %d taps %d", k.in,
          k.out, c.up, c.down, c.width, c.taps);
  }
  {
    int32_t a[6], b[6];
    for (int i = 0; i < 6; ++i) { a[i] = known[i].in; b[i] = known[i].out; }
    std::vector<char> img;
    std::string err;
    CHECK(build(a, b, 6, 6, 0.99, &img, &err), "known bank refused: %s", err.c_str());
    check_image(img, 6, "known bank");
    for (int i = 0; i < 5 && !img.empty(); ++i) {       // per-phase DC gain: the sum over the taps of one phase
      Conv c;
      memcpy(&c, img.data() + (16 + 8 * i) * 4, sizeof(c));
      for (int p = 0; p < c.up; ++p) {
        double s = 0.0;
        for (int k = 0; k < c.taps; ++k) {
          float v;
          memcpy(&v, img.data() + ((size_t)c.offset + (size_t)k * c.up + p) * 4, 4);
          s += v;
        }
        CHECK(s > 0.9999 && s < 1.0010, "%d -> %d phase %d: DC gain %.6f", known[i].in, known[i].out, p, s);
      }
    }
  }
  // ---- 2. hostile arguments
  {
    const int32_t ok_a[9] = {8000, 8000, 8000, 8000, 8000, 8000, 8000, 8000, 8000}, ok_b[9] = {16000, 16000, 16000, 16000, 16000, 16000, 16000, 16000, 16000};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    expect_error(nullptr, ok_b, 1, 6, 0.99, "null sr_in");
    expect_error(ok_a, nullptr, 1, 6, 0.99, "null sr_out");
    expect_error(ok_a, ok_b, 0, 6, 0.99, "no conversion");
    expect_error(ok_a, ok_b, -1, 6, 0.99, "negative count");
    expect_error(ok_a, ok_b, 9, 6, 0.99, "nine conversions");
    expect_error(ok_a, ok_b, 1, 0, 0.99, "lpw 0");
    expect_error(ok_a, ok_b, 1, 65, 0.99, "lpw 65");
    expect_error(ok_a, ok_b, 1, std::numeric_limits<int>::min(), 0.99, "lpw INT_MIN");
    expect_error(ok_a, ok_b, 1, std::numeric_limits<int>::max(), 0.99, "lpw INT_MAX");
    const double bad_roll[] = {0.0, -0.5, 1.0000001, 2.0, inf, -inf, nan, 4.9e-324, 1e-300, 1e-9};
    for (double r : bad_roll) expect_error(ok_a, ok_b, 1, 6, r, "rolloff");
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
    const int32_t bad[][2] = {{0, 16000}, {16000, 0}, {-1, 16000}, {16000, -16000}, {imin, imin}, {imax, imax - 1}, {imax, 1}, {1, imax},
                              {1025, 1}, {1, 1025}, {16000, 16001}, {44101, 16000}, {1023, 1024}};
    for (const auto& p : bad) expect_error(&p[0], &p[1], 1, 6, 0.99, "rates");
    const int32_t big_a = 1024, big_b = 1;               // 1/1024 at lpw 64: far more than 2^20 taps
    expect_error(&big_a, &big_b, 1, 64, 0.01, "tap count");
    // a short destination, a null destination
    std::string err;
    const size_t bytes = bank_bytes(ok_a, ok_b, 2, 6, 0.99, &err);
    CHECK(bytes > 0, "good bank refused");
    std::vector<char> dst(bytes ? bytes - 1 : 0);
    CHECK(bank_write(ok_a, ok_b, 2, 6, 0.99, dst.data(), dst.size(), &err) == kErrArg, "short destination accepted");
    CHECK(bank_write(ok_a, ok_b, 2, 6, 0.99, nullptr, bytes, &err) == kErrArg, "null destination accepted");
    // the extremes that ARE accepted: imax -> imax is the identity, 1 -> 1024 and 1024 -> 1 at the defaults
    const int32_t ea[3] = {imax, 1, 1024}, eb[3] = {imax, 1024, 1};
    std::vector<char> img;
    CHECK(build(ea, eb, 3, 6, 0.99, &img, &err), "extremes refused: %s", err.c_str());
    check_image(img, 3, "extremes");
  }
  // ---- 3. random draws
  int accepted = 0, refused = 0;
  for (int it = 0; it < 1000; ++it) {
    const int n = 1 + (int)(rnd() % 8);
    int32_t a[8], b[8];
    for (int i = 0; i < n; ++i) {
      const uint32_t mode = rnd() % 8;
      if (mode == 0) { a[i] = (int32_t)((int64_t)rnd() - (int64_t)(rnd() % 3) * 0x40000000LL); b[i] = (int32_t)rnd(); }       // anything, negatives included
      else if (mode == 1) { const int32_t g = 1 + (int32_t)(rnd() % 400); a[i] = g * (1 + (int32_t)(rnd() % 1100)); b[i] = g * (1 + (int32_t)(rnd() % 1100)); }
      else { a[i] = 1 + (int32_t)(rnd() % 64); b[i] = 1 + (int32_t)(rnd() % 64); }
    }
    const int lpw = (rnd() % 16 == 0) ? (int)(rnd() % 200) - 50 : 1 + (int)(rnd() % 64);
    const double rolloff = (rnd() % 16 == 0) ? ((double)(rnd() % 3000) - 500.0) / 1000.0 : (1.0 + (double)(rnd() % 1000)) / 1000.0;
    std::vector<char> img;
    std::string err;
    if (build(a, b, n, lpw, rolloff, &img, &err)) { ++accepted; check_image(img, n, "random bank"); }
    else { ++refused; CHECK(!err.empty(), "refusal without a message"); }
  }
  CHECK(accepted > 200 && refused > 200, "the corpus is one-sided: %d accepted, %d refused", accepted, refused);
  // ---- 4. out_len
  CHECK(out_len(0, 160, 441) == 0 && out_len(1, 160, 441) == 1 && out_len(441, 160, 441) == 160 && out_len(442, 160, 441) == 161, "out_len");
  CHECK(out_len(159999, 1, 3) == 53333 && out_len(160000, 10, 9) == 177778 && out_len(9, 10, 9) == 10, "out_len");
  CHECK(out_len(-1, 1, 1) == -1 && out_len(1, 0, 1) == -1 && out_len(1, 1, 0) == -1 && out_len(1, 1025, 1) == -1 && out_len(1, 1, 1025) == -1, "out_len refusals");
  CHECK(out_len(std::numeric_limits<int64_t>::max(), 1024, 1) == -1 && out_len(std::numeric_limits<int64_t>::max() / 1024, 1024, 1024) == -1, "out_len overflow");
  CHECK(out_len(std::numeric_limits<int64_t>::max() - 1, 1, 1) == std::numeric_limits<int64_t>::max() - 1, "out_len at the edge");
  fprintf(stderr, "fuzz corpus: %d banks accepted, %d refused\n", accepted, refused);
  if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
  printf("resample_fuzz ok\n");
  return 0;
}
