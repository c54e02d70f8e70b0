// Host side of the waveform augmentation (noise at a drawn SNR, reverberation with a room impulse response): the RIR bank of up to
// 256 impulse responses as ONE position-independent image (header table + taps) that the caller uploads and csrc/wave_aug.hip
// reads - plain C++17, no HIP header, so that the same source also builds as a g++ -fsanitize=address,undefined test binary
// (tests/sanitize/wave_aug_fuzz.cpp, run by tests/test_sanitize_wave_aug_cpu.py).  wave_aug.hip wraps these behind the C ABI
// (lasr_rir_bank_bytes / _bank_write).  The arguments are UNTRUSTED: every size is formed in int64 and checked before it is used.
//
// One RIR h[0..len) (DESIGN.md "Noise and reverberation"):
//   d = the first index of max |h|  (the direct path: the reverberated speech keeps its timing)
//   K = the smallest length >= d + 1 with sum_{k >= K} h[k]^2 <= 1e-6 * sum_k h[k]^2, at most kMaxTaps
//       (the sums in f64, each accumulated from the LAST sample towards the first)
//   y[j] = sum_{k < K} h[k] * x[j + d - k]
// Image layout (little endian, 4-byte words):
//   word 0 magic, word 1 number of RIRs, word 2 the image's size in words, word 3 zero, then 256 entries of 4 words
//   {K, d, offset of the taps in words from the image start, 0}; entries past the count are zero.
//   taps of an RIR: K f32 words, unscaled, followed by zeros up to the next multiple of kTapPad - the kernel walks the taps in
//   groups of kTapPad and a zero tap adds nothing.  Every offset is a multiple of 4 words.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <string>

namespace lasr {
namespace wave_aug {

constexpr uint32_t kMagic = 0x52495231u;      // "RIR1"
constexpr int kMaxRir = 256;
constexpr int kHeaderWords = 4 + 4 * kMaxRir;
constexpr int kMaxTaps = 8192;                // K
constexpr int64_t kMaxRirLen = 1 << 20;       // samples of one RIR handed to the builder
constexpr int64_t kMaxImageWords = 1 << 21;
constexpr int kTapPad = 8;                    // the kernel's inner loop: 2 groups of 4 taps
constexpr int kOutPerThread = 8;              // outputs a thread of the FIR keeps in registers: 4 consecutive ones in each half of the tile
constexpr int kTile = 256 * kOutPerThread;    // outputs per workgroup
constexpr int kChunk = 1536;                  // taps per staged chunk (a multiple of kTapPad): kTile + 2 kChunk f32 words of LDS
constexpr double kTailEnergy = 1e-6;
enum { kOk = 0, kErrArg = 1 };                // mapped to LASR_E_* by the wrappers

struct Entry {
  int32_t taps = 0, delay = 0, offset = 0, pad = 0;
};

constexpr int64_t padded(int64_t k) { return (k + kTapPad - 1) / kTapPad * kTapPad; }

static inline std::string at(int i, const char* what) { return "rir bank: RIR " + std::to_string(i) + " " + what; }

// geometry of RIR i (offset left 0)
static inline int plan(const float* h, int64_t len, int i, Entry* e, std::string* err) {
  if (len < 1) { *err = at(i, "is empty"); return kErrArg; }
  if (len > kMaxRirLen) { *err = at(i, "is longer than 2^20 samples"); return kErrArg; }
  if (!h) { *err = at(i, "is a null pointer"); return kErrArg; }
  float peak = 0.0f;
  int64_t d = 0;
  for (int64_t k = 0; k < len; ++k) {
    const float a = fabsf(h[k]);
    if (!(a <= 3.402823466e+38f)) { *err = at(i, "holds a value that is not finite"); return kErrArg; }   // NaN and inf
    if (a > peak) { peak = a; d = k; }
  }
  if (!(peak > 0.0f)) { *err = at(i, "is all zero"); return kErrArg; }
  if (d >= kMaxTaps) { *err = at(i, "has its peak at or past sample 8192"); return kErrArg; }
  double total = 0.0;
  for (int64_t k = len - 1; k >= 0; --k) total += (double)h[k] * (double)h[k];
  const double thr = kTailEnergy * total;
  int64_t K = len;
  double tail = 0.0;                                      // sum over k >= K
  while (K > d + 1) {
    const double t = tail + (double)h[K - 1] * (double)h[K - 1];
    if (!(t <= thr)) break;
    tail = t; --K;
  }
  if (K > kMaxTaps) K = kMaxTaps;
  *e = Entry();
  e->taps = (int32_t)K; e->delay = (int32_t)d;
  return kOk;
}

// rirs: the RIRs one after the other; lens[i] samples each
static inline int plan_all(const float* rirs, const int64_t* lens, int n_rir, Entry* ent, int64_t* words, std::string* err) {
  if (n_rir < 0 || n_rir > kMaxRir) { *err = "rir bank: a bank holds at most 256 RIRs"; return kErrArg; }
  if (n_rir && (!rirs || !lens)) { *err = "rir bank: null RIR list"; return kErrArg; }
  int64_t off = kHeaderWords, pos = 0;
  for (int i = 0; i < n_rir; ++i) {
    const int64_t len = lens[i];
    const int rc = plan(len >= 1 && len <= kMaxRirLen ? rirs + pos : nullptr, len, i, &ent[i], err);
    if (rc != kOk) return rc;
    ent[i].offset = (int32_t)off;
    off += padded(ent[i].taps);
    pos += len;
    if (off > kMaxImageWords) { *err = at(i, "takes the image above 2^21 words"); return kErrArg; }
  }
  *words = off;
  return kOk;
}

// size of the image in bytes; 0 (and *err) for arguments the bank does not take
static inline size_t bank_bytes(const float* rirs, const int64_t* lens, int n_rir, std::string* err) {
  Entry ent[kMaxRir];
  int64_t words = 0;
  if (plan_all(rirs, lens, n_rir, ent, &words, err) != kOk) return 0;
  return (size_t)words * 4;
}

static inline int bank_write(const float* rirs, const int64_t* lens, int n_rir, void* dst, size_t bytes, std::string* err) {
  Entry ent[kMaxRir];
  int64_t words = 0;
  const int rc = plan_all(rirs, lens, n_rir, ent, &words, err);
  if (rc != kOk) return rc;
  if (!dst || bytes < (size_t)words * 4) { *err = "rir bank: the destination is smaller than the bank image"; return kErrArg; }
  char* out = static_cast<char*>(dst);
  memset(out, 0, (size_t)words * 4);
  int32_t head[4] = {(int32_t)kMagic, n_rir, (int32_t)words, 0};
  memcpy(out, head, sizeof(head));
  int64_t pos = 0;
  for (int i = 0; i < n_rir; ++i) {
    memcpy(out + (size_t)(4 + 4 * i) * 4, &ent[i], sizeof(Entry));
    memcpy(out + (size_t)ent[i].offset * 4, rirs + pos, (size_t)ent[i].taps * 4);
    pos += lens[i];
  }
  return kOk;
}

// what csrc/wave_aug.hip requires of an entry before it reads a tap: also the check of the sanitizer program (constexpr: the
// kernel calls it too)
constexpr bool entry_ok(int32_t taps, int32_t delay, int32_t offset, int64_t image_words) {
  return taps >= 1 && taps <= kMaxTaps && delay >= 0 && delay < taps && offset >= kHeaderWords && (offset & 3) == 0 &&
         (int64_t)offset + padded(taps) <= image_words && image_words <= kMaxImageWords;
}

static_assert(sizeof(Entry) == 16, "a header entry is 4 words");
static_assert(kChunk % kTapPad == 0 && kTapPad % 4 == 0 && kHeaderWords % 4 == 0, "taps are read four at a time");

}  // namespace wave_aug
}  // namespace lasr
