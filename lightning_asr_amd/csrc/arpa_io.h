// Host-side reader of text ARPA n-gram language models and builder of the device image the LM-fused CTC beam search reads
// (ctc_beam.hip, lasr_ctc_beam_decode_lm) - plain C++17, no HIP header, so that the same source also builds as a
// g++ -fsanitize=address,undefined test binary (tests/sanitize/arpa_fuzz.cpp, run by tests/test_sanitize_arpa_cpu.py).
// ctc_beam.hip wraps it behind the C ABI (lasr_arpa_load / _info / _write_image / _free) and holds no parsing code.
//
// Accepted input: `\data\`, `ngram n=count` lines (orders 1..kArpaMaxOrder, consecutive from 1), one `\n-grams:` section per
// order in increasing order whose lines are `log10p w1 .. wn [log10bow]` separated by tabs or spaces, and `\end\`.  Text before
// `\data\` and after `\end\` is ignored, as are blank lines.  Rejected, with a message naming the line: malformed lines,
// non-finite numbers, counts that disagree with their section, duplicate n-grams, an n-gram whose suffix (w2..wn) is not stored
// (the device walk goes leftward from the last word one word at a time and needs suffix closure; KenLM's lmplz writes it),
// a missing `\end\`, and KenLM binary files (by their "mmap lm " magic).
//
// Device image (one contiguous block, all offsets from its start, little-endian):
//   ArpaImageHeader (64 bytes)
//   uni[n_words]   float2 (log10 p, log10 bow) per LM word id
//   cls[n_classes] int32  class -> LM word id, -1 = out of the LM's vocabulary (a string the ARPA lacks, or "<unk>")
//   slot[1 << log2_slots] ArpaSlot: open-addressing hash (linear probing) of every n-gram of order >= 2, keyed exactly by
//                  (index of its suffix w2..wn) << 32 | (LM word id of w1).  The index of an n-gram is its word id for a
//                  unigram and n_words + slot for a higher order, so a key never collides with another n-gram's.
// Only n-grams over words some vocabulary label maps to (plus <s> and </s>) are kept: no query can reach the others.
#pragma once
#include <cmath>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

namespace lasr {
namespace host {

constexpr int kArpaMaxOrder = 6;                 // KenLM's default limit
constexpr uint32_t kArpaImageMagic = 0x4d4c5341u;  // "ASLM"
constexpr uint64_t kArpaEmptyKey = ~0ull;
enum { kArpaOk = 0, kArpaErrOpen = 1, kArpaErrFormat = 2, kArpaErrUnsupported = 3, kArpaErrArg = 4 };

struct ArpaImageHeader {
  uint32_t magic, order, n_words, n_classes;
  uint32_t log2_slots, bos, eos, char_based;     // bos / eos: LM word ids of <s> / </s>, 0xFFFFFFFF when the LM lacks them
  uint64_t uni_off, cls_off, slot_off, n_ngrams;
};
static_assert(sizeof(ArpaImageHeader) == 64, "image header is 64 bytes");

struct ArpaSlot {
  uint64_t key;
  float lp, bow;
};
static_assert(sizeof(ArpaSlot) == 16, "one 16-byte load per probe");

// the slot a key starts probing at (splitmix64's finaliser); ctc_beam.hip carries the same function for the device
static inline uint64_t arpa_hash(uint64_t k) {
  k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
  k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

struct ArpaModel {
  int order = 0;
  bool char_based = false;
  int64_t n_ngrams = 0;            // n-grams kept in the image
  std::vector<unsigned char> image;
};

namespace arpa_detail {

static inline std::string at_line(int64_t line, const std::string& what) {
  return "line " + std::to_string((long long)line) + ": " + what;
}

static inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

static inline void split(const char* b, const char* e, std::vector<std::string>* out) {
  out->clear();
  while (b < e) {
    while (b < e && is_space(*b)) ++b;
    const char* s = b;
    while (b < e && !is_space(*b)) ++b;
    if (b > s) out->emplace_back(s, b);
  }
}

static inline bool parse_num(const std::string& s, float* v) {
  if (s.empty()) return false;
  char* end = nullptr;
  const double d = strtod(s.c_str(), &end);
  if (end != s.c_str() + s.size() || !std::isfinite(d) || fabs(d) > 1e30) return false;
  *v = (float)d;
  return true;
}

static inline bool parse_count(const char* s, int64_t* v) {
  if (*s < '0' || *s > '9') return false;
  int64_t x = 0;
  for (; *s >= '0' && *s <= '9'; ++s) {
    x = x * 10 + (*s - '0');
    if (x > (int64_t)1 << 40) return false;
  }
  while (is_space(*s)) ++s;
  *v = x;
  return *s == 0;
}

static inline int code_points(const std::string& w) {
  int n = 0;
  for (unsigned char ch : w) n += (ch & 0xC0) != 0x80;
  return n;
}

static inline bool special(const std::string& w) { return w == "<s>" || w == "</s>" || w == "<unk>"; }

}  // namespace arpa_detail

// Parses `text` (the whole file) and builds the device image for the class strings vocab[0 .. n_vocab).  Returns kArpaOk or an
// error code with *err set.
static inline int arpa_parse(const std::string& text, const char* const* vocab, int n_vocab, ArpaModel* m, std::string* err) {
  using namespace arpa_detail;
  if ((!vocab && n_vocab > 0) || n_vocab < 0 || !m) { *err = "null vocabulary or model"; return kArpaErrArg; }
  for (int i = 0; i < n_vocab; ++i)
    if (!vocab[i]) { *err = "vocabulary entry " + std::to_string(i) + " is null"; return kArpaErrArg; }
  if (text.compare(0, 8, "mmap lm ") == 0) { *err = "a KenLM binary model: only text ARPA files are read"; return kArpaErrUnsupported; }

  // full-file n-gram store: index = word id for unigrams, n_words + running count above
  std::unordered_map<std::string, uint32_t> wid;
  std::vector<std::string> words;
  std::unordered_map<uint64_t, uint32_t> idx;     // (suffix index << 32 | w1 id) -> index
  std::vector<float> lp, bow;
  std::vector<uint32_t> first, suffix;            // per index >= n_words: w1 id and suffix index
  std::vector<int64_t> declared;
  std::vector<std::string> tok;
  std::vector<uint32_t> ids;

  enum { kPre, kData, kSection, kEnd } state = kPre;
  int cur = 0;                                    // order of the current section
  int64_t in_section = 0, line = 0;
  size_t pos = 0;
  const size_t n = text.size();
  auto close_section = [&](int64_t ln) -> bool {
    if (cur > 0 && in_section != declared[cur - 1]) {
      *err = at_line(ln, "the " + std::to_string(cur) + "-gram section holds " + std::to_string((long long)in_section) +
                             " entries; \\data\\ declares " + std::to_string((long long)declared[cur - 1]));
      return false;
    }
    return true;
  };
  while (pos < n && state != kEnd) {
    size_t e = text.find('\n', pos);
    if (e == std::string::npos) e = n;
    const char* lb = text.data() + pos;
    const char* le = text.data() + e;
    pos = e + 1;
    ++line;
    while (lb < le && is_space(*lb)) ++lb;
    while (le > lb && is_space(le[-1])) --le;
    if (lb == le) continue;
    const std::string s(lb, le);
    if (state == kPre) {
      if (s == "\\data\\") state = kData;
      continue;
    }
    if (s[0] == '\\') {
      if (!close_section(line)) return kArpaErrFormat;
      if (s == "\\end\\") {
        if (cur != (int)declared.size()) { *err = at_line(line, "\\end\\ before every declared order had its section"); return kArpaErrFormat; }
        state = kEnd;
        break;
      }
      int64_t o = 0;
      const size_t tail = s.size() >= 8 ? s.size() - 7 : 0;
      if (tail < 2 || s.compare(tail, 7, "-grams:") != 0 || !parse_count(s.substr(1, tail - 1).c_str(), &o) ||
          o > kArpaMaxOrder) {
        *err = at_line(line, "unknown section header '" + s + "'");
        return kArpaErrFormat;
      }
      if (declared.empty()) { *err = at_line(line, "no 'ngram n=count' line in \\data\\"); return kArpaErrFormat; }
      if (o != cur + 1 || o > (int64_t)declared.size()) {
        *err = at_line(line, "section for order " + std::to_string(o) + " where order " + std::to_string(cur + 1) + " was due");
        return kArpaErrFormat;
      }
      cur = (int)o;
      in_section = 0;
      state = kSection;
      continue;
    }
    if (state == kData) {
      int64_t o = 0, c = 0;
      const size_t eq = s.find('=');
      if (s.compare(0, 6, "ngram ") != 0 || eq == std::string::npos) { *err = at_line(line, "expected 'ngram n=count'"); return kArpaErrFormat; }
      const std::string ostr = s.substr(6, eq - 6);
      const size_t o0 = ostr.find_first_not_of(" \t");
      if (o0 == std::string::npos || !parse_count(ostr.c_str() + o0, &o) || !parse_count(s.c_str() + eq + 1, &c)) {
        *err = at_line(line, "malformed 'ngram n=count'");
        return kArpaErrFormat;
      }
      if (o != (int64_t)declared.size() + 1) { *err = at_line(line, "orders must be declared in sequence from 1"); return kArpaErrFormat; }
      if (o > kArpaMaxOrder) {
        *err = at_line(line, "order " + std::to_string((long long)o) + " above the supported " + std::to_string(kArpaMaxOrder));
        return kArpaErrFormat;
      }
      declared.push_back(c);
      continue;
    }
    // an n-gram line of order cur
    split(lb, le, &tok);
    if ((int)tok.size() != cur + 1 && (int)tok.size() != cur + 2) {
      *err = at_line(line, "expected 'log10p w1 .. w" + std::to_string(cur) + " [log10bow]'");
      return kArpaErrFormat;
    }
    float p = 0.f, w = 0.f;
    if (!parse_num(tok[0], &p) || ((int)tok.size() == cur + 2 && !parse_num(tok.back(), &w))) {
      *err = at_line(line, "not a finite number");
      return kArpaErrFormat;
    }
    if (in_section >= declared[cur - 1]) {
      *err = at_line(line, "more " + std::to_string(cur) + "-grams than \\data\\ declares (" +
                               std::to_string((long long)declared[cur - 1]) + ")");
      return kArpaErrFormat;
    }
    ++in_section;
    if (cur == 1) {
      if (!wid.emplace(tok[1], (uint32_t)words.size()).second) { *err = at_line(line, "duplicate 1-gram '" + tok[1] + "'"); return kArpaErrFormat; }
      if (words.size() >= 0x7fffffffu) { *err = at_line(line, "too many words"); return kArpaErrFormat; }
      words.push_back(tok[1]);
      lp.push_back(p);
      bow.push_back(w);
      continue;
    }
    ids.resize(cur);
    for (int i = 0; i < cur; ++i) {
      auto it = wid.find(tok[1 + i]);
      if (it == wid.end()) { *err = at_line(line, "word '" + tok[1 + i] + "' is not a 1-gram: the n-gram's suffix is missing"); return kArpaErrFormat; }
      ids[i] = it->second;
    }
    const uint32_t nw = (uint32_t)words.size();
    uint32_t sfx = ids[cur - 1];
    for (int i = cur - 2; i >= 1; --i) {
      auto it = idx.find(((uint64_t)sfx << 32) | ids[i]);
      if (it == idx.end()) { *err = at_line(line, "the n-gram's suffix (its words 2.." + std::to_string(cur) + ") is not stored"); return kArpaErrFormat; }
      sfx = it->second;
    }
    const uint64_t key = ((uint64_t)sfx << 32) | ids[0];
    const uint64_t at = (uint64_t)nw + first.size();
    if (at >= 0x7fffffffu) { *err = at_line(line, "too many n-grams"); return kArpaErrFormat; }
    if (!idx.emplace(key, (uint32_t)at).second) { *err = at_line(line, "duplicate " + std::to_string(cur) + "-gram"); return kArpaErrFormat; }
    first.push_back(ids[0]);
    suffix.push_back(sfx);
    lp.push_back(p);
    bow.push_back(w);
  }
  if (state == kPre) { *err = "no \\data\\ section: not a text ARPA file"; return kArpaErrFormat; }
  if (state != kEnd) { *err = at_line(line, "the file ends before \\end\\"); return kArpaErrFormat; }
  if (declared.empty()) { *err = "no n-gram orders declared"; return kArpaErrFormat; }

  // ---- keep what the vocabulary can reach, build the image
  const uint32_t nw = (uint32_t)words.size();
  std::vector<int32_t> dev(nw, -1);
  std::vector<char> wanted(nw, 0);
  for (int i = 0; i < n_vocab; ++i) {
    auto it = wid.find(vocab[i]);
    if (it != wid.end() && words[it->second] != "<unk>") wanted[it->second] = 1;
  }
  bool char_based = true;
  uint32_t n_dev = 0, bos = 0xFFFFFFFFu, eos = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < nw; ++i) {
    if (!special(words[i]) && code_points(words[i]) != 1) char_based = false;
    if (words[i] == "<s>" || words[i] == "</s>") wanted[i] = 1;
    if (wanted[i]) {
      dev[i] = (int32_t)n_dev++;
      if (words[i] == "<s>") bos = (uint32_t)dev[i];
      if (words[i] == "</s>") eos = (uint32_t)dev[i];
    }
  }
  const size_t nh = first.size();
  std::vector<int64_t> dev_idx(nh, -1);
  size_t kept = 0;
  for (size_t j = 0; j < nh; ++j) {
    const uint32_t s = suffix[j];
    const bool sfx_kept = s < nw ? dev[s] >= 0 : dev_idx[s - nw] >= 0;
    if (dev[first[j]] >= 0 && sfx_kept) { dev_idx[j] = 0; ++kept; }
  }
  int log2_slots = 4;
  while (((size_t)1 << log2_slots) < 2 * kept) ++log2_slots;
  const size_t n_slots = (size_t)1 << log2_slots;
  auto align16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  ArpaImageHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = kArpaImageMagic;
  h.order = (uint32_t)declared.size();
  h.n_words = n_dev;
  h.n_classes = (uint32_t)n_vocab;
  h.log2_slots = (uint32_t)log2_slots;
  h.bos = bos;
  h.eos = eos;
  h.char_based = char_based ? 1u : 0u;
  h.uni_off = 64;
  h.cls_off = align16(h.uni_off + (size_t)n_dev * 8);
  h.slot_off = align16(h.cls_off + (size_t)n_vocab * 4);
  h.n_ngrams = n_dev + kept;
  std::vector<unsigned char> img((size_t)(h.slot_off + n_slots * sizeof(ArpaSlot)), 0);
  float* uni = reinterpret_cast<float*>(img.data() + h.uni_off);
  for (uint32_t i = 0; i < nw; ++i)
    if (dev[i] >= 0) { uni[2 * dev[i]] = lp[i]; uni[2 * dev[i] + 1] = bow[i]; }
  int32_t* cls = reinterpret_cast<int32_t*>(img.data() + h.cls_off);
  for (int i = 0; i < n_vocab; ++i) {
    auto it = wid.find(vocab[i]);
    cls[i] = (it != wid.end() && words[it->second] != "<unk>") ? dev[it->second] : -1;
  }
  ArpaSlot* slot = reinterpret_cast<ArpaSlot*>(img.data() + h.slot_off);
  for (size_t i = 0; i < n_slots; ++i) { slot[i].key = kArpaEmptyKey; slot[i].lp = 0.f; slot[i].bow = 0.f; }
  for (size_t j = 0; j < nh; ++j) {                // suffixes precede their extensions: their device index is known
    if (dev_idx[j] < 0) continue;
    const uint32_t s = suffix[j];
    const uint64_t sd = s < nw ? (uint64_t)dev[s] : (uint64_t)dev_idx[s - nw];
    const uint64_t key = (sd << 32) | (uint64_t)dev[first[j]];
    size_t at = (size_t)(arpa_hash(key) & (n_slots - 1));
    while (slot[at].key != kArpaEmptyKey) at = (at + 1) & (n_slots - 1);
    slot[at].key = key;
    slot[at].lp = lp[nw + j];
    slot[at].bow = bow[nw + j];
    dev_idx[j] = (int64_t)n_dev + (int64_t)at;
  }
  memcpy(img.data(), &h, sizeof(h));
  m->order = (int)declared.size();
  m->char_based = char_based;
  m->n_ngrams = (int64_t)h.n_ngrams;
  m->image.swap(img);
  return kArpaOk;
}

static inline int arpa_load(const char* path, const char* const* vocab, int n_vocab, ArpaModel* m, std::string* err) {
  if (!path) { *err = "null path"; return kArpaErrArg; }
  FILE* f = fopen(path, "rb");
  if (!f) { *err = std::string("cannot open ") + path; return kArpaErrOpen; }
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) { *err = std::string("cannot read ") + path; return kArpaErrOpen; }
  const int rc = arpa_parse(text, vocab, n_vocab, m, err);
  if (rc != kArpaOk) *err = std::string(path) + ": " + *err;
  return rc;
}

}  // namespace host
}  // namespace lasr
