// Host side of the resampler: the polyphase windowed-sinc filter bank of up to 8 rate conversions as ONE position-independent image
// (header table + taps) that the caller uploads and csrc/resample.hip reads - plain C++17, no HIP header, so that the same source
// also builds as a g++ -fsanitize=address,undefined test binary (tests/sanitize/resample_fuzz.cpp, run by
// tests/test_sanitize_resample_cpu.py).  resample.hip wraps these behind the C ABI (lasr_resample_bank_bytes / _bank_write /
// _out_len).  The arguments are UNTRUSTED: every product is formed in int64 / double and checked before it sizes anything.
//
// One conversion (sr_in, sr_out), lpw = 6 and rolloff = 0.99 by default (DESIGN.md "Resampling"):
//   g = gcd(sr_in, sr_out); down = sr_in / g; up = sr_out / g; base = min(up, down) * rolloff
//   width = ceil(lpw * down / base); taps = 2 * width + down
//   h[p][k] = (base / down) * sinc(t) * cos(pi t / (2 lpw))^2,  t = clamp(((k - width) / down - p / up) * base, -lpw, +lpw)
//   out[j] = sum_k h[j % up][k] * x[(j / up) * down + k - width]  (x = 0 outside the row),  n_out = ceil(n_in * up / down)
// Taps are computed in f64 and rounded once to f32.  Image layout (little endian, 4-byte words):
//   word 0 magic, word 1 number of conversions, words 2..15 zero, then 8 entries of 8 words
//   {up, down, width, taps, offset of the taps in words from the image start, nblk, kc, 0};  entries past the count are zero.
//   taps of a conversion: [tap k][phase p] = word offset + k * up + p, so that consecutive outputs read consecutive words.
//   nblk / kc are the kernel's tiling of this conversion: a workgroup produces nblk * up consecutive outputs (nblk input blocks
//   of `down` samples) and walks the taps in chunks of kc, with (nblk - 1) * down + kc <= kSpanCap samples staged per chunk.
// An identity conversion (up == down == 1) has taps = 0 and no words of its own: the kernel copies such rows.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

namespace lasr {
namespace resample {

constexpr uint32_t kMagic = 0x52534d31u;      // "RSM1"
constexpr int kMaxConv = 8;
constexpr int kHeaderWords = 16 + 8 * kMaxConv;
constexpr int64_t kMaxFactor = 1024;          // up, down
constexpr int64_t kMaxBankWords = 1 << 20;    // up * taps of one conversion
constexpr int kSpanCap = 8192;                // input samples a workgroup stages per tap chunk (32 KB of LDS as f32)
constexpr int kMaxChunk = 4096;               // taps per chunk
constexpr int kMaxTile = 1024;                // outputs per workgroup: 256 threads x 4 accumulators
enum { kOk = 0, kErrArg = 1 };                // mapped to LASR_E_* by the wrappers

struct Conv {
  int32_t up = 0, down = 0, width = 0, taps = 0, offset = 0, nblk = 0, kc = 0, pad = 0;
};

static inline int64_t gcd64(int64_t a, int64_t b) {
  while (b) { const int64_t t = a % b; a = b; b = t; }
  return a;
}

// n_out = ceil(n_in * up / down) in integer arithmetic; -1 for arguments outside the supported range
static inline int64_t out_len(int64_t n_in, int64_t up, int64_t down) {
  if (n_in < 0 || up < 1 || down < 1 || up > kMaxFactor || down > kMaxFactor || n_in > (INT64_MAX - down) / up) return -1;
  return (n_in * up + down - 1) / down;
}

// geometry of one conversion (offset left 0)
static inline int plan(int64_t sr_in, int64_t sr_out, int lpw, double rolloff, Conv* c, std::string* err) {
  if (sr_in < 1 || sr_out < 1) { *err = "resample: sample rates must be positive"; return kErrArg; }
  if (!(rolloff > 0.0 && rolloff <= 1.0)) { *err = "resample: rolloff must lie in (0, 1]"; return kErrArg; }
  if (lpw < 1 || lpw > 64) { *err = "resample: lpw (low-pass filter width) must lie in [1, 64]"; return kErrArg; }
  const int64_t g = gcd64(sr_in, sr_out);
  const int64_t down = sr_in / g, up = sr_out / g;
  if (up > kMaxFactor || down > kMaxFactor) {
    *err = "resample: " + std::to_string((long long)sr_in) + " -> " + std::to_string((long long)sr_out) + " reduces to " +
           std::to_string((long long)up) + "/" + std::to_string((long long)down) + ", above 1024";
    return kErrArg;
  }
  *c = Conv();
  c->up = (int32_t)up; c->down = (int32_t)down;
  if (up == 1 && down == 1) { c->nblk = kMaxTile; return kOk; }      // identity: a copy, no filter
  const double base = (double)(up < down ? up : down) * rolloff;
  const double w = ceil((double)lpw * (double)down / base);
  const double taps = 2.0 * w + (double)down;
  if (!(taps * (double)up <= (double)kMaxBankWords)) {               // also refuses a NaN / inf from a denormal rolloff
    *err = "resample: " + std::to_string((long long)up) + "/" + std::to_string((long long)down) + " needs more than 2^20 filter taps";
    return kErrArg;
  }
  c->width = (int32_t)w; c->taps = (int32_t)taps;
  c->kc = c->taps < kMaxChunk ? c->taps : kMaxChunk;
  int64_t nblk = (kSpanCap - c->kc) / down + 1;
  if (nblk > kMaxTile / up) nblk = kMaxTile / up;
  c->nblk = (int32_t)(nblk < 1 ? 1 : nblk);
  return kOk;
}

static inline int plan_all(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff, Conv* convs, int64_t* words,
                           std::string* err) {
  if (!sr_in || !sr_out) { *err = "resample: null rate list"; return kErrArg; }
  if (n_conv < 1 || n_conv > kMaxConv) { *err = "resample: a bank holds 1 to 8 conversions"; return kErrArg; }
  int64_t off = kHeaderWords;
  for (int i = 0; i < n_conv; ++i) {
    const int rc = plan(sr_in[i], sr_out[i], lpw, rolloff, &convs[i], err);
    if (rc != kOk) return rc;
    convs[i].offset = (int32_t)off;
    off += (int64_t)convs[i].up * convs[i].taps;          // <= 8 * 2^20 words in all
  }
  *words = off;
  return kOk;
}

static inline double tap(const Conv& c, int lpw, double rolloff, int p, int k) {
  const double kPi = 3.14159265358979323846;
  const double base = (double)(c.up < c.down ? c.up : c.down) * rolloff;
  double t = ((double)(k - c.width) / (double)c.down - (double)p / (double)c.up) * base;
  t = t < -(double)lpw ? -(double)lpw : (t > (double)lpw ? (double)lpw : t);
  const double win = cos(kPi * t / (2.0 * (double)lpw));
  const double sinc = t == 0.0 ? 1.0 : sin(kPi * t) / (kPi * t);
  return (base / (double)c.down) * sinc * win * win;
}

// size of the image in bytes; 0 (and *err) for arguments the bank does not take
static inline size_t bank_bytes(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff, std::string* err) {
  Conv convs[kMaxConv];
  int64_t words = 0;
  if (plan_all(sr_in, sr_out, n_conv, lpw, rolloff, convs, &words, err) != kOk) return 0;
  return (size_t)words * 4;
}

static inline int bank_write(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff, void* dst, size_t bytes,
                             std::string* err) {
  Conv convs[kMaxConv];
  int64_t words = 0;
  const int rc = plan_all(sr_in, sr_out, n_conv, lpw, rolloff, convs, &words, err);
  if (rc != kOk) return rc;
  if (!dst || bytes < (size_t)words * 4) { *err = "resample: the destination is smaller than the bank image"; return kErrArg; }
  char* out = static_cast<char*>(dst);
  int32_t head[kHeaderWords];
  memset(head, 0, sizeof(head));
  head[0] = (int32_t)kMagic; head[1] = n_conv;
  for (int i = 0; i < n_conv; ++i) memcpy(head + 16 + 8 * i, &convs[i], sizeof(Conv));
  memcpy(out, head, sizeof(head));
  for (int i = 0; i < n_conv; ++i) {
    const Conv& c = convs[i];
    char* base = out + (size_t)c.offset * 4;
    for (int k = 0; k < c.taps; ++k)
      for (int p = 0; p < c.up; ++p) {
        const float v = (float)tap(c, lpw, rolloff, p, k);
        memcpy(base + ((size_t)k * c.up + p) * 4, &v, 4);
      }
  }
  return kOk;
}

static_assert(sizeof(Conv) == 32, "a header entry is 8 words");

}  // namespace resample
}  // namespace lasr
