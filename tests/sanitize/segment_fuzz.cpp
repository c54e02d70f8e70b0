// CPU sanitizer pass over the host side of the voice-activity segmenter: built by tests/test_sanitize_segment_cpu.py as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/sanitize/segment_fuzz.cpp
// against lightning_asr_amd/csrc/segment.h - the SAME source liblasr.so compiles (segment.hip wraps it, and its kernels call level()).
// No GPU, no HIP.  Exit code 0 = every case behaved (a clean error or parameters inside what the kernels rely on); any sanitizer
// report aborts with a non-zero code.
//
//   1. level(): 0 for 0, monotone and below 512 over all powers of two, their neighbours and the maximum energy of a frame; eight
//      levels per octave; against a bit-by-bit reference;
//   2. known answers of the conversion: the defaults and the small parameters of the tests;
//   3. the dB -> steps -> dB round trip within one step, seconds -> frames -> seconds within one frame;
//   4. hostile arguments - NaN, +-inf, negative and huge dB and seconds, permille outside 1..1000, off above on, min_level above
//      max_floor_level, max_frames below 2 - each a clean error; 100 000 LCG-driven draws: refused, or a struct that check() takes;
//   5. lengths: zero, one frame more or less, 2^31 - 1, 2^31, negative.
#include "../../lightning_asr_amd/csrc/segment.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace lasr::segment;

static int g_fail = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

static uint64_t g_lcg = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_lcg >> 33); }

static int level_ref(uint64_t e) {            // the rule, one bit at a time
  if (!e) return 0;
  int k = 0;
  for (uint64_t t = e; t > 1; t >>= 1) ++k;
  int m = 0;
  for (int j = 1; j <= 3; ++j) m = 2 * m + (k - j >= 0 ? (int)((e >> (k - j)) & 1) : 0);
  return 8 * k + m + 1;
}

static void check_levels() {
  CHECK(level(0) == 0 && level(1) == 1, "level(0), level(1)");
  int prev = 0;
  uint64_t prev_e = 0;
  for (int k = 0; k < 64; ++k)
    for (int d = -1; d <= 1; ++d) {
      const uint64_t e = ((uint64_t)1 << k) + (uint64_t)(int64_t)d;
      if (e == 0 || (k == 0 && d < 0)) continue;
      const int lv = level(e);
      CHECK(lv == level_ref(e), "level(2^%d%+d) = %d, reference %d", k, d, lv, level_ref(e));
      CHECK(lv < kLevels, "level(2^%d%+d) = %d", k, d, lv);
      if (e >= prev_e) CHECK(lv >= prev, "level not monotone at 2^%d%+d", k, d);
      if (d == 0 && k > 0) CHECK(lv - level((uint64_t)1 << (k - 1)) == 8, "an octave is eight levels at 2^%d", k);
      prev = lv; prev_e = e;
    }
  CHECK(level(kMaxEnergy) == 8 * 37 + 2 + 1 && level(kMaxEnergy) < kLevels, "level of the loudest frame: %d", level(kMaxEnergy));
  CHECK(level(kMaxEnergy - 1) <= level(kMaxEnergy) && level(kMaxEnergy + 1) >= level(kMaxEnergy), "neighbours of the loudest frame");
  for (int i = 0; i < 100000; ++i) {
    const uint64_t e = (((uint64_t)rnd() << 32) | rnd()) >> (rnd() % 64);
    CHECK(level(e) == level_ref(e), "level(%llu)", (unsigned long long)e);
    if (e < ~(uint64_t)0) CHECK(level(e + 1) >= level(e), "level not monotone at %llu", (unsigned long long)e);
  }
}

static void check_known() {
  Params p;
  std::string err;
  CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kOk, "defaults refused: %s", err.c_str());
  CHECK(p.on_steps == 32 && p.off_steps == 16 && p.floor_permille == 100 && p.min_level == 139 && p.max_floor_level == 205 &&
        p.min_silence == 30 && p.min_speech == 10 && p.pad == 10 && p.max_frames == 1600, "defaults: %d %d %d %d %d %d %d %d %d", p.on_steps,
        p.off_steps, p.floor_permille, p.min_level, p.max_floor_level, p.min_silence, p.min_speech, p.pad, p.max_frames);
  CHECK(from(12.0, 6.0, 100, -1000.0, 0.0, 0.03, 0.02, 0.01, 0.08, &p, &err) == kOk, "small parameters refused: %s", err.c_str());
  CHECK(p.min_level == 0 && p.max_floor_level == level(kMaxEnergy) && p.min_silence == 3 && p.min_speech == 2 && p.pad == 1 && p.max_frames == 8,
        "small parameters");
  CHECK(num_frames(0) == 0 && num_frames(1) == 1 && num_frames(159) == 1 && num_frames(160) == 1 && num_frames(161) == 2 &&
        num_frames(-5) == 0 && num_frames(kMaxLen) == 13421773, "num_frames");
}

static void check_round_trips() {
  std::string err;
  for (int i = 0; i <= 40000; ++i) {
    const double db = -100.0 + i * 0.005;
    int32_t s = 0;
    CHECK(steps_from_db(db, "db", &s, &err) == kOk, "steps_from_db(%g)", db);
    CHECK(fabs(s * kStepDb - db) <= 0.5 * kStepDb + 1e-12, "dB round trip at %g: %d steps", db, s);
  }
  for (int i = 0; i <= 20000; ++i) {
    const double sec = i * 0.0037;
    int32_t f = 0;
    CHECK(frames_from_seconds(sec, "s", &f, &err) == kOk, "frames_from_seconds(%g)", sec);
    CHECK(fabs(f / kFramesPerSecond - sec) <= 0.5 / kFramesPerSecond + 1e-9, "seconds round trip at %g: %d frames", sec, f);
  }
  int32_t lo = 0, hi = 0;
  for (int i = 0; i <= 1000; ++i) {           // an absolute level rises with its dBFS
    CHECK(level_from_dbfs(-100.0 + 0.1 * i, "l", &hi, &err) == kOk, "level_from_dbfs");
    CHECK(hi >= lo && hi < kLevels, "absolute level not monotone at %g dBFS", -100.0 + 0.1 * i);
    lo = hi;
  }
}

static bool inside(const Params& p) {
  std::string err;
  return check(p, &err) == kOk && p.off_steps >= 0 && p.off_steps <= p.on_steps && p.floor_permille >= 1 && p.floor_permille <= 1000 &&
         p.min_level >= 0 && p.min_level <= p.max_floor_level && p.max_floor_level < kLevels && p.min_silence >= 0 && p.min_speech >= 0 &&
         p.pad >= 0 && p.max_frames >= 2 && p.max_frames <= (1 << 30);
}

static void check_hostile() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double bad[] = {nan, inf, -inf, 1e300, -1e300, 1e9, -1e9, std::numeric_limits<double>::max()};
  Params p;
  std::string err;
  for (double v : bad) {
    err.clear();
    CHECK(from(v, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg && !err.empty(), "on_db %g accepted", v);
    CHECK(from(12.0, v, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "off_db %g accepted", v);
    CHECK(from(12.0, 6.0, 100, v, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "min_level_db %g accepted", v);
    CHECK(from(12.0, 6.0, 100, -60.0, v, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "max_floor_db %g accepted", v);
    CHECK(from(12.0, 6.0, 100, -60.0, -35.0, v, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "min_silence_s %g accepted", v);
    CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, v, 0.1, 16.0, &p, &err) == kErrArg, "min_speech_s %g accepted", v);
    CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, 0.1, v, 16.0, &p, &err) == kErrArg, "pad_s %g accepted", v);
    CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, v, &p, &err) == kErrArg, "max_segment_s %g accepted", v);
  }
  CHECK(from(1000.0001, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "on_db above 1000 accepted");
  CHECK(from(12.0, 6.0, 100, -1000.0001, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "min_level_db below -1000 accepted");
  CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 1000000.5, &p, &err) == kErrArg, "max_segment_s above 1e6 accepted");
  CHECK(from(12.0, 6.0, 100, -60.0, -35.0, -0.001, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "negative seconds accepted");
  CHECK(from(12.0, 6.0, 100, -60.0, 0.5, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "a floor above 0 dBFS accepted");
  CHECK(from(6.0, 12.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "off above on accepted");
  CHECK(from(12.0, -1.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "negative off accepted");
  CHECK(from(12.0, 6.0, 100, -35.0, -60.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "min_level above max_floor_level accepted");
  CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 0.014, &p, &err) == kErrArg, "max_frames 1 accepted");
  CHECK(from(12.0, 6.0, 100, -60.0, -35.0, 0.3, 0.1, 0.1, 0.0, &p, &err) == kErrArg, "max_frames 0 accepted");
  const int64_t permille[] = {0, -1, 1001, INT64_MIN, INT64_MAX, (int64_t)1 << 32};
  for (int64_t v : permille) CHECK(from(12.0, 6.0, v, -60.0, -35.0, 0.3, 0.1, 0.1, 16.0, &p, &err) == kErrArg, "floor_permille %lld accepted", (long long)v);
  CHECK(from(12.0, 6.0, 1, -60.0, -35.0, 0.0, 0.0, 0.0, 0.02, &p, &err) == kOk && inside(p), "the smallest parameters refused: %s", err.c_str());
  CHECK(from(1000.0, 1000.0, 1000, -1000.0, 0.0, 1e6, 1e6, 1e6, 1e6, &p, &err) == kOk && inside(p), "the largest parameters refused: %s", err.c_str());
  // a struct filled in by hand goes through check()
  const Params good = {32, 16, 100, 139, 205, 30, 10, 10, 1600};
  CHECK(check(good, &err) == kOk, "a good struct refused");
  for (int f = 0; f < 9; ++f)
    for (int32_t v : {INT32_MIN, -1, INT32_MAX}) {
      Params q = good;
      int32_t* w = &q.on_steps + f;
      *w = v;
      CHECK(check(q, &err) == kErrArg, "field %d = %d accepted", f, v);
    }
  int ok = 0, refused = 0;
  for (int i = 0; i < 100000; ++i) {
    auto draw = [&](double lo, double hi) {
      const uint32_t k = rnd() % 16;
      if (k == 0) return bad[rnd() % (sizeof(bad) / sizeof(bad[0]))];
      if (k == 1) return lo - 1e-9 * (1 + rnd() % 1000);
      if (k == 2) return hi + 1e-9 * (1 + rnd() % 1000);
      return lo + (hi - lo) * (rnd() / 2147483648.0);
    };
    const int rc = from(draw(0.0, 60.0), draw(0.0, 30.0), (int64_t)(rnd() % 1100) - 50, draw(-120.0, 0.0), draw(-120.0, 0.0), draw(0.0, 5.0),
                        draw(0.0, 5.0), draw(0.0, 5.0), draw(0.0, 100.0), &p, &err);
    if (rc == kOk) { ++ok; CHECK(inside(p), "draw %d: accepted parameters outside the kernels' range", i); }
    else { ++refused; CHECK(rc == kErrArg && !err.empty(), "draw %d: return code %d", i, rc); }
  }
  fprintf(stderr, "fuzz corpus: %d accepted, %d refused\n", ok, refused);
  CHECK(ok > 1000 && refused > 1000, "the draws do not cover both outcomes");
}

static void check_lengths() {
  std::string err;
  const int64_t good[] = {0, 1, 159, 160, 161, kMaxLen};
  for (int64_t v : good) CHECK(check_len(v, &err) == kOk, "length %lld refused", (long long)v);
  const int64_t badl[] = {-1, kMaxLen + 1, INT64_MAX, INT64_MIN};
  for (int64_t v : badl) CHECK(check_len(v, &err) == kErrArg, "length %lld accepted", (long long)v);
  CHECK(num_frames(kMaxLen) * (int64_t)kHop >= kMaxLen && num_frames(kMaxLen) < (1 << 24), "frames of the longest row");
}

int main() {
  check_levels();
  check_known();
  check_round_trips();
  check_hostile();
  check_lengths();
  if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
  printf("segment_fuzz ok\n");
  return 0;
}
