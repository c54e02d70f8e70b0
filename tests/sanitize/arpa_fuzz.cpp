// CPU sanitizer pass over the ARPA reader: built by tests/test_sanitize_arpa_cpu.py as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/sanitize/arpa_fuzz.cpp
// against lightning_asr_amd/csrc/arpa_io.h - the SAME source liblasr.so compiles (ctc_beam.hip wraps it).  No GPU, no HIP.
// Exit code 0 = every case behaved (a clean error or a consistent image); any sanitizer report aborts with a non-zero code.
//
//   1. a good file loads and its image is self-consistent (offsets inside the image, every probe chain ends on an empty slot);
//   2. every truncation of that file, 3 000 LCG-driven byte mutations, line deletions and duplications, hostile counts and
//      orders, numbers that overflow, KenLM's binary magic, an empty file and a file of NUL bytes: each either loads into a
//      consistent image or fails with a message, never crashes.
#include "../../lightning_asr_amd/csrc/arpa_io.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace lasr::host;

static int g_fail = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

static const char* kGood =
    "\\data\\\nngram 1=6\nngram 2=5\nngram 3=2\n\n"
    "\\1-grams:\n-99\t<s>\t-0.3\n-0.7\t</s>\n-0.5\ta\t-0.2\n-0.6\tb\t-0.25\n-0.9\tc\t-0.1\n-1.0\t<unk>\n\n"
    "\\2-grams:\n-0.4\t<s> a\t-0.1\n-0.3\ta b\t-0.15\n-0.35\tb a\t-0.05\n-0.2\tb </s>\n-0.5 c a -0.3\n\n"
    "\\3-grams:\n-0.1\t<s> a b\n-0.12\ta b a\n\n\\end\\\n";

static const char* kVocab[] = {"a", "b", "c", "d", "<unk>", "\xe4\xb8\x80"};
static const int kNVocab = 6;

// the image's internal consistency: what the kernel relies on before it reads it
static void check_image(const ArpaModel& m, const char* what) {
  CHECK(m.image.size() >= sizeof(ArpaImageHeader), "%s: image too small", what);
  if (m.image.size() < sizeof(ArpaImageHeader)) return;
  ArpaImageHeader h;
  memcpy(&h, m.image.data(), sizeof(h));
  const size_t n_slots = (size_t)1 << h.log2_slots;
  CHECK(h.magic == kArpaImageMagic && h.order >= 1 && h.order <= (uint32_t)kArpaMaxOrder, "%s: header", what);
  CHECK(h.uni_off + (size_t)h.n_words * 8 <= h.cls_off && h.cls_off + (size_t)h.n_classes * 4 <= h.slot_off &&
            h.slot_off + n_slots * sizeof(ArpaSlot) == m.image.size(), "%s: offsets", what);
  CHECK(h.n_classes == (uint32_t)kNVocab, "%s: classes", what);
  const int32_t* cls = reinterpret_cast<const int32_t*>(m.image.data() + h.cls_off);
  for (uint32_t i = 0; i < h.n_classes; ++i) CHECK(cls[i] >= -1 && cls[i] < (int32_t)h.n_words, "%s: class map", what);
  const ArpaSlot* slot = reinterpret_cast<const ArpaSlot*>(m.image.data() + h.slot_off);
  size_t used = 0;
  for (size_t i = 0; i < n_slots; ++i) {
    if (slot[i].key == kArpaEmptyKey) continue;
    ++used;
    const uint64_t sfx = slot[i].key >> 32, w = slot[i].key & 0xffffffffu;
    CHECK(w < h.n_words && sfx < h.n_words + n_slots, "%s: key", what);
    CHECK(sfx < h.n_words || slot[sfx - h.n_words].key != kArpaEmptyKey, "%s: suffix slot", what);
  }
  CHECK(2 * used <= n_slots, "%s: load factor", what);
  CHECK(used + h.n_words == h.n_ngrams, "%s: n-gram count", what);
}

static void run(const std::string& text, const char* what, bool must_load) {
  ArpaModel m;
  std::string err;
  const int rc = arpa_parse(text, kVocab, kNVocab, &m, &err);
  if (rc == kArpaOk) check_image(m, what);
  else CHECK(!err.empty(), "%s: error without a message", what);
  if (must_load) CHECK(rc == kArpaOk, "%s: rc %d (%s)", what, rc, err.c_str());
}

static uint64_t g_lcg = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}

int main(int argc, char** argv) {
  const std::string good = kGood;
  run(good, "good", true);
  {
    ArpaModel m;
    std::string err;
    CHECK(arpa_parse(good, kVocab, kNVocab, &m, &err) == kArpaOk && m.order == 3 && m.char_based, "good: info");
  }
  int n = 0;
  for (size_t cut = 0; cut < good.size(); ++cut, ++n) run(good.substr(0, cut), "truncation", false);
  const char* const specials[] = {"nan", "inf", "-inf", "1e999", "ngram 9=1", "ngram 1=99999999999999999999", "\\7-grams:",
                                  "\\-1-grams:", "\\99999999999-grams:", "\\data\\", "\\end\\", "", "\t", " ", "x y z w v u t",
                                  "-0.5\tzz\t-0.2", "ngram 1=", "=", "ngram =3"};
  for (int i = 0; i < 3000; ++i, ++n) {
    std::string t = good;
    const int op = rnd() % 5;
    const size_t at = rnd() % t.size();
    if (op == 0) t[at] = (char)(rnd() & 255);
    else if (op == 1) t.erase(at, 1 + rnd() % 8);
    else if (op == 2) t.insert(at, specials[rnd() % (sizeof(specials) / sizeof(specials[0]))]);
    else if (op == 3) {                                              // delete a whole line
      const size_t b = t.rfind('\n', at), e = t.find('\n', at);
      if (b != std::string::npos && e != std::string::npos) t.erase(b, e - b);
    } else {                                                         // duplicate a whole line
      const size_t b = t.rfind('\n', at), e = t.find('\n', at);
      if (b != std::string::npos && e != std::string::npos) t.insert(e, t.substr(b, e - b));
    }
    run(t, "mutation", false);
  }
  run("", "empty", false);
  run(std::string(4096, '\0'), "nul bytes", false);
  run(std::string("mmap lm http://kheafield.com/code format version 5\n") + std::string(64, '\0'), "kenlm binary", false);
  run("\\data\\\nngram 1=1\n\n\\1-grams:\n-1\ta\n\\end\\\n", "no <s>", true);
  n += 4;
  // the file path: a missing file and the good file through arpa_load
  if (argc > 1) {
    const std::string p = std::string(argv[1]) + "/good.arpa";
    FILE* f = fopen(p.c_str(), "wb");
    if (f) { fwrite(good.data(), 1, good.size(), f); fclose(f); }
    ArpaModel m;
    std::string err;
    CHECK(arpa_load(p.c_str(), kVocab, kNVocab, &m, &err) == kArpaOk, "arpa_load good: %s", err.c_str());
    CHECK(arpa_load((std::string(argv[1]) + "/missing.arpa").c_str(), kVocab, kNVocab, &m, &err) == kArpaErrOpen, "missing");
    CHECK(arpa_load(nullptr, kVocab, kNVocab, &m, &err) == kArpaErrArg, "null path");
  }
  fprintf(stderr, "fuzz corpus: %d files\n", n);
  if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
  printf("arpa_fuzz ok\n");
  return 0;
}
