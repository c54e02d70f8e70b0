// Host side of the voice-activity segmenter: the quasi-log level of a frame's energy, the conversion of its parameters from dB and
// seconds to the integers the kernels take, and their range checks - plain C++17, no HIP header, so that the same source also builds
// as a g++ -fsanitize=address,undefined test binary (tests/sanitize/segment_fuzz.cpp, run by tests/test_sanitize_segment_cpu.py).
// segment.hip wraps these behind the C ABI (lasr_vad_params_from / lasr_vad_segment) and its kernels call level() themselves (a
// constexpr function: the one definition serves both sides).  The arguments are UNTRUSTED: every value is checked as a double
// before it is cast.  The rule itself is stated in DESIGN.md "Inference: long recordings".
//
//   frame n = samples [160 n, 160 n + 160) of the row, E[n] = sum of q^2 over it (q = the PCM16 value), at most 160 * 2^30
//   level(E) = 0 for E == 0, else 8 k + m + 1 with k = floor(log2 E) and m = the three bits of E below its leading one:
//   8 steps per octave of power, one step = 10 log10(2) / 8 = 0.376 dB, monotone in E
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string>

namespace lasr {
namespace segment {

constexpr int kHop = 160;                               // samples per frame: the mel hop
constexpr int kLevels = 512;                            // histogram bins (LASR_VAD_LEVELS); level(E) < 512 for every E < 15 * 2^59
constexpr uint64_t kMaxEnergy = (uint64_t)kHop << 30;   // 160 samples of -32768
constexpr double kStepDb = 10.0 * 0.30102999566398119521 / 8.0;
constexpr double kFramesPerSecond = 16000.0 / kHop;
constexpr double kMaxDb = 1000.0;                       // |dB| a relative threshold may have; an absolute one lies in [-1000, 0] dBFS
constexpr double kMaxSeconds = 1.0e6;                   // 10^8 frames: every frame count stays far inside int32
constexpr int64_t kMaxLen = ((int64_t)1 << 31) - 1;     // samples of one row
enum { kOk = 0, kErrArg = 1 };                          // mapped to LASR_E_* by the wrappers

struct Params {                                         // lasr_vad_params, field for field
  int32_t on_steps, off_steps, floor_permille, min_level, max_floor_level, min_silence, min_speech, pad, max_frames;
};

constexpr int level(uint64_t e) {
  if (e == 0) return 0;
  const int k = 63 - __builtin_clzll(e);
  const uint64_t m = (k >= 3 ? e >> (k - 3) : e << (3 - k)) & 7;
  return 8 * k + (int)m + 1;
}

static inline int64_t num_frames(int64_t len) { return len <= 0 ? 0 : (len + kHop - 1) / kHop; }

static inline int check_len(int64_t len, std::string* err) {
  if (len < 0 || len > kMaxLen) { *err = "vad: a row holds 0 to 2^31 - 1 samples"; return kErrArg; }
  return kOk;
}

// relative dB -> level steps, rounded half to even
static inline int steps_from_db(double db, const char* what, int32_t* out, std::string* err) {
  if (!(db >= -kMaxDb && db <= kMaxDb)) { *err = std::string("vad: ") + what + " must be a finite number of dB within +-1000"; return kErrArg; }
  *out = (int32_t)rint(db / kStepDb);
  return kOk;
}

// absolute dBFS of a full frame -> level: 0 dBFS is a frame of 160 samples at full scale
static inline int level_from_dbfs(double db, const char* what, int32_t* out, std::string* err) {
  if (!(db >= -kMaxDb && db <= 0.0)) { *err = std::string("vad: ") + what + " must lie in [-1000, 0] dBFS"; return kErrArg; }
  const double e = rint((double)kMaxEnergy * pow(10.0, db / 10.0));        // in [0, 160 * 2^30]
  *out = level((uint64_t)e);
  return kOk;
}

static inline int frames_from_seconds(double s, const char* what, int32_t* out, std::string* err) {
  if (!(s >= 0.0 && s <= kMaxSeconds)) { *err = std::string("vad: ") + what + " must lie in [0, 1e6] seconds"; return kErrArg; }
  *out = (int32_t)rint(s * kFramesPerSecond);
  return kOk;
}

// what the kernels rely on; also applied to a struct the caller filled in by hand
static inline int check(const Params& p, std::string* err) {
  const int32_t cap = 1 << 30;
  if (!(0 <= p.off_steps && p.off_steps <= p.on_steps && p.on_steps <= cap)) { *err = "vad: need 0 <= off_steps <= on_steps"; return kErrArg; }
  if (p.floor_permille < 1 || p.floor_permille > 1000) { *err = "vad: floor_permille must lie in 1..1000"; return kErrArg; }
  if (!(0 <= p.min_level && p.min_level <= p.max_floor_level && p.max_floor_level < kLevels)) {
    *err = "vad: need 0 <= min_level <= max_floor_level < 512";
    return kErrArg;
  }
  if (p.min_silence < 0 || p.min_silence > cap || p.min_speech < 0 || p.min_speech > cap || p.pad < 0 || p.pad > cap) {
    *err = "vad: min_silence, min_speech and pad are frame counts in [0, 2^30]";
    return kErrArg;
  }
  if (p.max_frames < 2 || p.max_frames > cap) { *err = "vad: max_frames must lie in [2, 2^30]"; return kErrArg; }
  return kOk;
}

static inline int from(double on_db, double off_db, int64_t floor_permille, double min_level_db, double max_floor_db, double min_silence_s,
                       double min_speech_s, double pad_s, double max_segment_s, Params* p, std::string* err) {
  *p = Params();
  if (floor_permille < 1 || floor_permille > 1000) { *err = "vad: floor_permille must lie in 1..1000"; return kErrArg; }
  p->floor_permille = (int32_t)floor_permille;
  if (steps_from_db(on_db, "on_db", &p->on_steps, err) != kOk || steps_from_db(off_db, "off_db", &p->off_steps, err) != kOk ||
      level_from_dbfs(min_level_db, "min_level_db", &p->min_level, err) != kOk ||
      level_from_dbfs(max_floor_db, "max_floor_db", &p->max_floor_level, err) != kOk ||
      frames_from_seconds(min_silence_s, "min_silence_s", &p->min_silence, err) != kOk ||
      frames_from_seconds(min_speech_s, "min_speech_s", &p->min_speech, err) != kOk ||
      frames_from_seconds(pad_s, "pad_s", &p->pad, err) != kOk ||
      frames_from_seconds(max_segment_s, "max_segment_s", &p->max_frames, err) != kOk)
    return kErrArg;
  return check(*p, err);
}

static_assert(sizeof(Params) == 36, "nine int32 fields");
static_assert(level(kMaxEnergy) < kLevels && level(1) == 1 && level(8) == 25 && level(15) == 32 && level(16) == 33, "the level rule");

}  // namespace segment
}  // namespace lasr
