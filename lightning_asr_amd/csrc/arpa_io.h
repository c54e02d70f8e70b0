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
//
// Word-level files (arpa_parse_words / arpa_load_words, for lasr_ctc_beam_decode_wlm): the same uni / cls / slot sections under
// another magic (kArpaWordImageMagic, so that each search kernel rejects the other kind of image), kept for the SPELLABLE words
// - every code point a one-code-point, non-space label - plus <s> and </s>; cls is all -1 (a label is no LM word here).  An
// ArpaLexHeader (64 bytes) follows the ArpaImageHeader and names the lexicon appended behind the slots:
//   edge[1 << log2_edges] ArpaLexEdge: open-addressing hash (linear probing, load <= 1/2) keyed exactly by
//                  (trie node << 32 | class id) -> child node; node 0 is the root
//   node_word[n_nodes] int32: LM word id of the word a node spells, -1 for a node that is no complete word
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
constexpr uint32_t kArpaWordImageMagic = 0x574c5341u;  // "ASLW"
constexpr uint64_t kArpaEmptyKey = ~0ull;
enum { kArpaOk = 0, kArpaErrOpen = 1, kArpaErrFormat = 2, kArpaErrUnsupported = 3, kArpaErrArg = 4 };

struct ArpaImageHeader {
  uint32_t magic, order, n_words, n_classes;
  uint32_t log2_slots, bos, eos, char_based;     // bos / eos: LM word ids of <s> / </s>, 0xFFFFFFFF when the LM lacks them
  uint64_t uni_off, cls_off, slot_off, n_ngrams;
};
static_assert(sizeof(ArpaImageHeader) == 64, "image header is 64 bytes");

struct ArpaLexHeader {                           // at byte 64 of a word image
  uint64_t edge_off, node_off;
  uint32_t log2_edges, n_nodes, space_id, n_lexicon_words, n_dropped_words;
  uint32_t reserved[7];
};
static_assert(sizeof(ArpaLexHeader) == 64, "lexicon header is 64 bytes");

struct ArpaLexEdge {
  uint64_t key;                                  // node << 32 | class, kArpaEmptyKey when free
  int32_t child, reserved;
};
static_assert(sizeof(ArpaLexEdge) == 16, "one 16-byte load per probe");

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
  bool word_mode = false;          // built by arpa_parse_words, which also sets the three counts below
  int64_t n_lexicon_words = 0, n_nodes = 0, n_dropped_words = 0;
  std::vector<unsigned char> image;
};

// a text ARPA file as read: an n-gram's index is its word id for a unigram, n_words + running count above
struct ArpaFile {
  std::unordered_map<std::string, uint32_t> wid;
  std::vector<std::string> words;
  std::vector<float> lp, bow;
  std::vector<uint32_t> first, suffix;            // per index >= n_words: w1 id and suffix index
  int order = 0;
  bool char_based = true;
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

// the checks every build makes before it reads the text
static inline int arpa_check_args(const std::string& text, const char* const* vocab, int n_vocab, const ArpaModel* m,
                                  std::string* err) {
  if ((!vocab && n_vocab > 0) || n_vocab < 0 || !m) { *err = "null vocabulary or model"; return kArpaErrArg; }
  for (int i = 0; i < n_vocab; ++i)
    if (!vocab[i]) { *err = "vocabulary entry " + std::to_string(i) + " is null"; return kArpaErrArg; }
  if (text.compare(0, 8, "mmap lm ") == 0) { *err = "a KenLM binary model: only text ARPA files are read"; return kArpaErrUnsupported; }
  return kArpaOk;
}

// Parses `text` (the whole file) into *f and checks suffix closure.  Returns kArpaOk or kArpaErrFormat with *err set.
static inline int arpa_read(const std::string& text, ArpaFile* f, std::string* err) {
  using namespace arpa_detail;
  std::unordered_map<std::string, uint32_t>& wid = f->wid;
  std::vector<std::string>& words = f->words;
  std::unordered_map<uint64_t, uint32_t> idx;     // (suffix index << 32 | w1 id) -> index
  std::vector<float>&lp = f->lp, &bow = f->bow;
  std::vector<uint32_t>&first = f->first, &suffix = f->suffix;
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
  f->order = (int)declared.size();
  f->char_based = true;
  for (const std::string& w : words)
    if (!special(w) && code_points(w) != 1) f->char_based = false;
  return kArpaOk;
}

// Builds the header and the uni / cls / slot sections, the first of them head_bytes into the image, over the words with
// wanted[file word id] set (<s> and </s> are added) and the class -> file word id map cls_word (-1: none).  (*dev_out)[file
// word id] is the word's LM id in the image, -1 when it was left out.
static inline void arpa_build_ngrams(const ArpaFile& f, std::vector<char> wanted, const std::vector<int64_t>& cls_word,
                                     uint32_t magic, size_t head_bytes, ArpaModel* m, std::vector<int32_t>* dev_out) {
  const std::vector<std::string>& words = f.words;
  const std::vector<float>&lp = f.lp, &bow = f.bow;
  const std::vector<uint32_t>&first = f.first, &suffix = f.suffix;
  const int n_vocab = (int)cls_word.size();
  const bool char_based = f.char_based;
  const uint32_t nw = (uint32_t)words.size();
  std::vector<int32_t> dev(nw, -1);
  uint32_t n_dev = 0, bos = 0xFFFFFFFFu, eos = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < nw; ++i) {
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
  h.magic = magic;
  h.order = (uint32_t)f.order;
  h.n_words = n_dev;
  h.n_classes = (uint32_t)n_vocab;
  h.log2_slots = (uint32_t)log2_slots;
  h.bos = bos;
  h.eos = eos;
  h.char_based = char_based ? 1u : 0u;
  h.uni_off = head_bytes;
  h.cls_off = align16(h.uni_off + (size_t)n_dev * 8);
  h.slot_off = align16(h.cls_off + (size_t)n_vocab * 4);
  h.n_ngrams = n_dev + kept;
  std::vector<unsigned char> img((size_t)(h.slot_off + n_slots * sizeof(ArpaSlot)), 0);
  float* uni = reinterpret_cast<float*>(img.data() + h.uni_off);
  for (uint32_t i = 0; i < nw; ++i)
    if (dev[i] >= 0) { uni[2 * dev[i]] = lp[i]; uni[2 * dev[i] + 1] = bow[i]; }
  int32_t* cls = reinterpret_cast<int32_t*>(img.data() + h.cls_off);
  for (int i = 0; i < n_vocab; ++i) cls[i] = cls_word[i] >= 0 ? dev[cls_word[i]] : -1;
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
  m->order = f.order;
  m->char_based = char_based;
  m->n_ngrams = (int64_t)h.n_ngrams;
  m->image.swap(img);
  if (dev_out) dev_out->swap(dev);
}

// Parses `text` (the whole file) and builds the device image for the class strings vocab[0 .. n_vocab).  Returns kArpaOk or an
// error code with *err set.
static inline int arpa_parse(const std::string& text, const char* const* vocab, int n_vocab, ArpaModel* m, std::string* err) {
  int rc = arpa_check_args(text, vocab, n_vocab, m, err);
  if (rc != kArpaOk) return rc;
  ArpaFile f;
  rc = arpa_read(text, &f, err);
  if (rc != kArpaOk) return rc;
  // keep what the vocabulary can reach
  std::vector<char> wanted(f.words.size(), 0);
  std::vector<int64_t> cls_word((size_t)n_vocab, -1);
  for (int i = 0; i < n_vocab; ++i) {
    auto it = f.wid.find(vocab[i]);
    if (it != f.wid.end() && f.words[it->second] != "<unk>") { wanted[it->second] = 1; cls_word[i] = it->second; }
  }
  arpa_build_ngrams(f, wanted, cls_word, kArpaImageMagic, sizeof(ArpaImageHeader), m, nullptr);
  return kArpaOk;
}

// The word-level build: `text` must be a word-level file and vocab[space_id] the vocabulary's only " " label (otherwise
// kArpaErrUnsupported).  Keeps the spellable words, builds the n-gram sections over them and appends the lexicon trie.  A label
// string that occurs twice spells with its first class.
static inline int arpa_parse_words(const std::string& text, const char* const* vocab, int n_vocab, int space_id, ArpaModel* m,
                                   std::string* err) {
  using namespace arpa_detail;
  int rc = arpa_check_args(text, vocab, n_vocab, m, err);
  if (rc != kArpaOk) return rc;
  int n_space = 0;
  for (int i = 0; i < n_vocab; ++i) n_space += strcmp(vocab[i], " ") == 0;
  if (space_id < 0 || space_id >= n_vocab || strcmp(vocab[space_id], " ") != 0 || n_space != 1) {
    *err = "a word-level LM needs exactly one \" \" label and space_id " + std::to_string(space_id) + " is not it";
    return kArpaErrUnsupported;
  }
  ArpaFile f;
  rc = arpa_read(text, &f, err);
  if (rc != kArpaOk) return rc;
  if (f.char_based) { *err = "a character-level LM: the word-level build takes a file with words of several code points"; return kArpaErrUnsupported; }
  std::unordered_map<std::string, int32_t> label;           // one-code-point, non-space label -> class
  for (int i = 0; i < n_vocab; ++i) {
    const std::string s = vocab[i];
    if (i != space_id && !s.empty() && (s[0] & 0xC0) != 0x80 && code_points(s) == 1) label.emplace(s, i);
  }
  // the trie over the spellable words, in file order; a word's code points are the runs (lead byte, continuation bytes)
  const uint32_t nw = (uint32_t)f.words.size();
  std::vector<char> wanted(nw, 0);
  std::unordered_map<uint64_t, uint32_t> edge;
  std::vector<int64_t> node_file_word(1, -1);                // node -> file word id
  std::vector<int32_t> spell;
  int64_t n_lex = 0, n_drop = 0;
  for (uint32_t i = 0; i < nw; ++i) {
    const std::string& w = f.words[i];
    if (special(w)) continue;
    spell.clear();
    bool ok = !w.empty();
    for (size_t a = 0; ok && a < w.size();) {
      size_t b = a + 1;
      while (b < w.size() && (w[b] & 0xC0) == 0x80) ++b;
      auto it = label.find(w.substr(a, b - a));
      if (it == label.end()) ok = false;
      else spell.push_back(it->second);
      a = b;
    }
    if (!ok) { ++n_drop; continue; }
    uint32_t node = 0;
    for (int32_t c : spell) {
      const uint64_t key = ((uint64_t)node << 32) | (uint32_t)c;
      auto it = edge.find(key);
      if (it == edge.end()) {
        if (node_file_word.size() >= 0x7fffffffu) { *err = "the lexicon needs more than 2^31 - 1 trie nodes"; return kArpaErrFormat; }
        it = edge.emplace(key, (uint32_t)node_file_word.size()).first;
        node_file_word.push_back(-1);
      }
      node = it->second;
    }
    node_file_word[node] = i;                                // words are distinct strings: no node is claimed twice
    wanted[i] = 1;
    ++n_lex;
  }
  std::vector<int32_t> dev;
  const std::vector<int64_t> cls_word((size_t)n_vocab, -1);
  arpa_build_ngrams(f, wanted, cls_word, kArpaWordImageMagic, sizeof(ArpaImageHeader) + sizeof(ArpaLexHeader), m, &dev);
  int log2_edges = 4;
  while (((size_t)1 << log2_edges) < 2 * edge.size()) ++log2_edges;
  const size_t n_edges = (size_t)1 << log2_edges, n_nodes = node_file_word.size();
  ArpaLexHeader lh;
  memset(&lh, 0, sizeof(lh));
  lh.edge_off = (m->image.size() + 15) & ~(size_t)15;
  lh.node_off = lh.edge_off + n_edges * sizeof(ArpaLexEdge);
  lh.log2_edges = (uint32_t)log2_edges;
  lh.n_nodes = (uint32_t)n_nodes;
  lh.space_id = (uint32_t)space_id;
  lh.n_lexicon_words = (uint32_t)n_lex;
  lh.n_dropped_words = (uint32_t)n_drop;
  m->image.resize((size_t)lh.node_off + n_nodes * sizeof(int32_t), 0);
  memcpy(m->image.data() + sizeof(ArpaImageHeader), &lh, sizeof(lh));
  ArpaLexEdge* e = reinterpret_cast<ArpaLexEdge*>(m->image.data() + lh.edge_off);
  for (size_t i = 0; i < n_edges; ++i) { e[i].key = kArpaEmptyKey; e[i].child = -1; e[i].reserved = 0; }
  for (const auto& kv : edge) {
    size_t at = (size_t)(arpa_hash(kv.first) & (n_edges - 1));
    while (e[at].key != kArpaEmptyKey) at = (at + 1) & (n_edges - 1);
    e[at].key = kv.first;
    e[at].child = (int32_t)kv.second;
  }
  int32_t* nwd = reinterpret_cast<int32_t*>(m->image.data() + lh.node_off);
  for (size_t i = 0; i < n_nodes; ++i) nwd[i] = node_file_word[i] >= 0 ? dev[node_file_word[i]] : -1;
  m->word_mode = true;
  m->n_lexicon_words = n_lex;
  m->n_nodes = (int64_t)n_nodes;
  m->n_dropped_words = n_drop;
  return kArpaOk;
}

static inline int arpa_read_file(const char* path, std::string* text, std::string* err) {
  if (!path) { *err = "null path"; return kArpaErrArg; }
  FILE* f = fopen(path, "rb");
  if (!f) { *err = std::string("cannot open ") + path; return kArpaErrOpen; }
  char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text->append(buf, got);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) { *err = std::string("cannot read ") + path; return kArpaErrOpen; }
  return kArpaOk;
}

static inline int arpa_load(const char* path, const char* const* vocab, int n_vocab, ArpaModel* m, std::string* err) {
  std::string text;
  int rc = arpa_read_file(path, &text, err);
  if (rc != kArpaOk) return rc;
  rc = arpa_parse(text, vocab, n_vocab, m, err);
  if (rc != kArpaOk) *err = std::string(path) + ": " + *err;
  return rc;
}

static inline int arpa_load_words(const char* path, const char* const* vocab, int n_vocab, int space_id, ArpaModel* m,
                                  std::string* err) {
  std::string text;
  int rc = arpa_read_file(path, &text, err);
  if (rc != kArpaOk) return rc;
  rc = arpa_parse_words(text, vocab, n_vocab, space_id, m, err);
  if (rc != kArpaOk) *err = std::string(path) + ": " + *err;
  return rc;
}

}  // namespace host
}  // namespace lasr
