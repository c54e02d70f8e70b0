// CPU sanitizer pass over the word-mode image builder (arpa_parse_words / arpa_load_words): built by
// tests/test_sanitize_arpa_words_cpu.py as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/sanitize/arpa_words_fuzz.cpp
// against lightning_asr_amd/csrc/arpa_io.h - the SAME source liblasr.so compiles (ctc_beam.hip wraps it).  No GPU, no HIP.
// Exit code 0 = every case behaved (a clean error or a consistent image); any sanitizer report aborts with a non-zero code.
//
//   1. a good word-level file loads; its image is walked fully: the n-gram slots, then the lexicon from the root over every
//      (node, class) with no probe leaving the table, every child and word id in range, every node reached exactly once;
//   2. every truncation of that file, 3 000 LCG-driven byte and line mutations, a word of 5 000 code points (spellable, and
//      with one code point that is not), words of invalid UTF-8 (stray continuation bytes, cut sequences, 0xFF), hostile
//      vocabularies (duplicate labels, multi-code-point labels, an empty label, invalid UTF-8 labels) and space ids: each
//      either loads into a consistent image or fails with a message, never crashes.
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
    "\\data\\\nngram 1=9\nngram 2=6\nngram 3=2\n\n"
    "\\1-grams:\n-99\t<s>\t-0.3\n-0.7\t</s>\n-0.5\ta\t-0.2\n-0.6\tab\t-0.25\n-0.9\tabba\t-0.1\n-0.8\tb\xe4\xb8\x80\t-0.1\n"
    "-1.1\tax\t-0.2\n-1.2\taa\n-1.0\t<unk>\n\n"
    "\\2-grams:\n-0.4\t<s> a\t-0.1\n-0.3\ta ab\t-0.15\n-0.35\tab a\t-0.05\n-0.2\tab </s>\n-0.5 abba a -0.3\n-0.6 ax a\n\n"
    "\\3-grams:\n-0.1\t<s> a ab\n-0.12\ta ab a\n\n\\end\\\n";

static const char* kVocab[] = {" ", "a", "b", "c", "\xe4\xb8\x80", "<unk>", "a"};   // a multi-code-point label, a duplicate
static const int kNVocab = 7;

// walks the whole image as the kernel may: returns false (after a CHECK) on the first inconsistency
static void check_image(const ArpaModel& m, const char* const* vocab, int n_vocab, const char* what) {
  const size_t head = sizeof(ArpaImageHeader) + sizeof(ArpaLexHeader);
  CHECK(m.word_mode && !m.char_based && m.image.size() >= head, "%s: model", what);
  if (m.image.size() < head) return;
  ArpaImageHeader h;
  ArpaLexHeader lh;
  memcpy(&h, m.image.data(), sizeof(h));
  memcpy(&lh, m.image.data() + sizeof(h), sizeof(lh));
  const size_t n_slots = (size_t)1 << h.log2_slots, n_edges = (size_t)1 << lh.log2_edges;
  CHECK(h.magic == kArpaWordImageMagic && h.order >= 1 && h.order <= (uint32_t)kArpaMaxOrder && h.char_based == 0, "%s: header", what);
  CHECK(h.uni_off == head && h.uni_off + (size_t)h.n_words * 8 <= h.cls_off && h.cls_off + (size_t)h.n_classes * 4 <= h.slot_off &&
            h.slot_off + n_slots * sizeof(ArpaSlot) <= lh.edge_off && lh.edge_off % 16 == 0 &&
            lh.edge_off + n_edges * sizeof(ArpaLexEdge) == lh.node_off &&
            lh.node_off + (size_t)lh.n_nodes * 4 == m.image.size(), "%s: offsets", what);
  CHECK(h.n_classes == (uint32_t)n_vocab && lh.space_id < (uint32_t)n_vocab && strcmp(vocab[lh.space_id], " ") == 0, "%s: classes", what);
  CHECK(lh.n_nodes >= 1 && (int64_t)lh.n_nodes == m.n_nodes && (int64_t)lh.n_lexicon_words == m.n_lexicon_words &&
            (int64_t)lh.n_dropped_words == m.n_dropped_words, "%s: counts", what);
  if (g_fail) return;
  const int32_t* cls = reinterpret_cast<const int32_t*>(m.image.data() + h.cls_off);
  for (uint32_t i = 0; i < h.n_classes; ++i) CHECK(cls[i] == -1, "%s: class map", what);
  const ArpaSlot* slot = reinterpret_cast<const ArpaSlot*>(m.image.data() + h.slot_off);
  size_t used = 0;
  for (size_t i = 0; i < n_slots; ++i) {
    if (slot[i].key == kArpaEmptyKey) continue;
    ++used;
    const uint64_t sfx = slot[i].key >> 32, w = slot[i].key & 0xffffffffu;
    CHECK(w < h.n_words && sfx < h.n_words + n_slots, "%s: key", what);
    CHECK(sfx < h.n_words || slot[sfx - h.n_words].key != kArpaEmptyKey, "%s: suffix slot", what);
  }
  CHECK(2 * used <= n_slots && used + h.n_words == h.n_ngrams, "%s: n-gram slots", what);
  // the lexicon: a breadth-first walk from the root over every class, probing as the kernel does
  const ArpaLexEdge* edge = reinterpret_cast<const ArpaLexEdge*>(m.image.data() + lh.edge_off);
  const int32_t* node_word = reinterpret_cast<const int32_t*>(m.image.data() + lh.node_off);
  size_t e_used = 0;
  for (size_t i = 0; i < n_edges; ++i) e_used += edge[i].key != kArpaEmptyKey;
  CHECK(2 * e_used <= n_edges && e_used + 1 == lh.n_nodes, "%s: edge load (a trie has one edge per node but the root)", what);
  std::vector<char> seen(lh.n_nodes, 0);
  std::vector<char> word_seen(h.n_words, 0);
  std::vector<uint32_t> queue(1, 0);
  seen[0] = 1;
  size_t words = 0, walked = 0;
  for (size_t qi = 0; qi < queue.size(); ++qi) {
    const uint32_t node = queue[qi];
    const int32_t w = node_word[node];
    CHECK(w >= -1 && w < (int32_t)h.n_words && (node != 0 || w == -1), "%s: node word", what);
    if (w >= 0 && w < (int32_t)h.n_words) {
      CHECK(!word_seen[w] && (uint32_t)w != h.bos && (uint32_t)w != h.eos, "%s: a word id on two nodes, or <s> / </s>", what);
      word_seen[w] = 1;
      ++words;
    }
    for (int c = 0; c < n_vocab + 1; ++c) {
      const uint64_t key = ((uint64_t)node << 32) | (uint32_t)c;
      size_t at = (size_t)(arpa_hash(key) & (n_edges - 1)), steps = 0;
      while (edge[at].key != key && edge[at].key != kArpaEmptyKey && steps <= n_edges) { at = (at + 1) & (n_edges - 1); ++steps; }
      CHECK(steps <= n_edges, "%s: a probe went round the table", what);
      if (steps > n_edges || edge[at].key != key) continue;
      const int32_t ch = edge[at].child;
      CHECK(c != (int)lh.space_id && c < n_vocab && ch > 0 && (uint32_t)ch < lh.n_nodes && !seen[ch], "%s: edge", what);
      if (ch > 0 && (uint32_t)ch < lh.n_nodes && !seen[ch]) { seen[ch] = 1; queue.push_back((uint32_t)ch); ++walked; }
    }
  }
  CHECK(queue.size() == lh.n_nodes && walked == e_used, "%s: %zu of %u nodes reached", what, queue.size(), lh.n_nodes);
  CHECK(words == lh.n_lexicon_words && words + 2 >= h.n_words && words <= h.n_words, "%s: lexicon words", what);
}

static int run(const std::string& text, const char* const* vocab, int n_vocab, int space_id, const char* what, bool must_load) {
  ArpaModel m;
  std::string err;
  const int rc = arpa_parse_words(text, vocab, n_vocab, space_id, &m, &err);
  if (rc == kArpaOk) check_image(m, vocab, n_vocab, what);
  else CHECK(!err.empty(), "%s: error without a message", what);
  if (must_load) CHECK(rc == kArpaOk, "%s: rc %d (%s)", what, rc, err.c_str());
  return rc;
}

static uint64_t g_lcg = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}

static std::string unigram_file(const std::vector<std::string>& words) {
  std::string t = "\\data\\\nngram 1=" + std::to_string(words.size() + 2) + "\n\n\\1-grams:\n-99\t<s>\t-0.3\n-0.7\t</s>\n";
  for (const std::string& w : words) t += "-1.5\t" + w + "\n";
  return t + "\n\\end\\\n";
}

int main(int argc, char** argv) {
  const std::string good = kGood;
  run(good, kVocab, kNVocab, 0, "good", true);
  {
    ArpaModel m;
    std::string err;
    CHECK(arpa_parse_words(good, kVocab, kNVocab, 0, &m, &err) == kArpaOk && m.order == 3 && !m.char_based, "good: info");
    // a ab abba aa b<U+4E00> spell; ax does not ("x" is no label)
    CHECK(m.n_lexicon_words == 5 && m.n_dropped_words == 1 && m.n_nodes == 1 + 4 + 1 + 2, "good: %lld words %lld dropped %lld nodes",
          (long long)m.n_lexicon_words, (long long)m.n_dropped_words, (long long)m.n_nodes);
    CHECK(m.n_ngrams == 7 + 5 + 2, "good: %lld n-grams kept", (long long)m.n_ngrams);
  }
  int n = 1;
  for (size_t cut = 0; cut < good.size(); ++cut, ++n) run(good.substr(0, cut), kVocab, kNVocab, 0, "truncation", false);
  const char* const specials[] = {"nan", "inf", "1e999", "ngram 9=1", "ngram 1=99999999999999999999", "\\7-grams:", "\\data\\",
                                  "\\end\\", "", "\t", " ", "\x80", "\xe4\xb8", "\xff\xfe", "-0.5\tzz\t-0.2", "-0.5\t\x80\x80\t-0.2",
                                  "-0.5\ta\xe4\t-0.2", "ngram 1=", "="};
  for (int i = 0; i < 3000; ++i, ++n) {
    std::string t = good;
    const int op = rnd() % 5;
    const size_t at = rnd() % t.size();
    if (op == 0) t[at] = (char)(rnd() & 255);
    else if (op == 1) t.erase(at, 1 + rnd() % 8);
    else if (op == 2) t.insert(at, specials[rnd() % (sizeof(specials) / sizeof(specials[0]))]);
    else if (op == 3) {
      const size_t b = t.rfind('\n', at), e = t.find('\n', at);
      if (b != std::string::npos && e != std::string::npos) t.erase(b, e - b);
    } else {
      const size_t b = t.rfind('\n', at), e = t.find('\n', at);
      if (b != std::string::npos && e != std::string::npos) t.insert(e, t.substr(b, e - b));
    }
    run(t, kVocab, kNVocab, 0, "mutation", false);
  }
  // a word of 5 000 code points: spellable (a chain of 5 000 nodes), and with one code point no label has
  {
    std::string longw;
    for (int i = 0; i < 5000; ++i) longw += (i % 3 == 2) ? "\xe4\xb8\x80" : (i % 3 ? "b" : "a");
    ArpaModel m;
    std::string err;
    CHECK(arpa_parse_words(unigram_file({longw, "ba"}), kVocab, kNVocab, 0, &m, &err) == kArpaOk && m.n_lexicon_words == 2 &&
              m.n_nodes == 1 + 5000 + 2, "long word: %s", err.c_str());
    run(unigram_file({longw, "ba"}), kVocab, kNVocab, 0, "long word", true);
    std::string bad = longw;
    bad.insert(2500 * 5 / 3, "x");
    CHECK(arpa_parse_words(unigram_file({bad, "ba"}), kVocab, kNVocab, 0, &m, &err) == kArpaOk && m.n_lexicon_words == 1 &&
              m.n_dropped_words == 1 && m.n_nodes == 3, "long unspellable word");
    n += 3;
  }
  // invalid UTF-8 in words: none spells, all are dropped, the image stays consistent
  {
    const std::vector<std::string> words = {"ab", "\x80", "\x80\x80" "a", "a\xe4", "a\xe4\xb8", "\xe4\xb8\x80\x80", "\xff\xfe", "a\xc0\xaf",
                                            "\xf0\x9f\x98", "b\xed\xa0\x80"};
    ArpaModel m;
    std::string err;
    CHECK(arpa_parse_words(unigram_file(words), kVocab, kNVocab, 0, &m, &err) == kArpaOk && m.n_lexicon_words == 1 &&
              m.n_dropped_words == (int64_t)words.size() - 1, "invalid UTF-8 words: %lld kept", (long long)m.n_lexicon_words);
    run(unigram_file(words), kVocab, kNVocab, 0, "invalid utf-8", true);
    n += 2;
  }
  // hostile vocabularies and space ids
  {
    const char* two_spaces[] = {" ", "a", " "};
    const char* no_space[] = {"a", "b"};
    const char* odd[] = {"", "\x80", "ab", " ", "\xe4\xb8", "a", "\xff"};
    CHECK(run(good, two_spaces, 3, 0, "two spaces", false) == kArpaErrUnsupported, "two spaces");
    CHECK(run(good, no_space, 2, 0, "no space", false) == kArpaErrUnsupported, "no space");
    CHECK(run(good, kVocab, kNVocab, -1, "space -1", false) == kArpaErrUnsupported, "space -1");
    CHECK(run(good, kVocab, kNVocab, kNVocab, "space n", false) == kArpaErrUnsupported, "space n");
    CHECK(run(good, kVocab, kNVocab, 1, "space 1", false) == kArpaErrUnsupported, "space 1");
    CHECK(run(good, odd, 7, 3, "odd labels", true) == kArpaOk, "odd labels");
    CHECK(run(good, nullptr, 3, 0, "null vocab", false) == kArpaErrArg, "null vocab");
    const std::string chars = "\\data\\\nngram 1=3\n\n\\1-grams:\n-99\t<s>\n-1\t</s>\n-1\ta\n\n\\end\\\n";
    CHECK(run(chars, kVocab, kNVocab, 0, "character file", false) == kArpaErrUnsupported, "character file");
    run("", kVocab, kNVocab, 0, "empty", false);
    run(std::string(4096, '\0'), kVocab, kNVocab, 0, "nul bytes", false);
    CHECK(run(std::string("mmap lm http://kheafield.com/code format version 5\n") + std::string(64, '\0'), kVocab, kNVocab, 0,
              "kenlm binary", false) == kArpaErrUnsupported, "kenlm binary");
    n += 11;
  }
  if (argc > 1) {
    const std::string p = std::string(argv[1]) + "/good_words.arpa";
    FILE* f = fopen(p.c_str(), "wb");
    if (f) { fwrite(good.data(), 1, good.size(), f); fclose(f); }
    ArpaModel m;
    std::string err;
    CHECK(arpa_load_words(p.c_str(), kVocab, kNVocab, 0, &m, &err) == kArpaOk, "arpa_load_words good: %s", err.c_str());
    CHECK(arpa_load_words((std::string(argv[1]) + "/missing.arpa").c_str(), kVocab, kNVocab, 0, &m, &err) == kArpaErrOpen, "missing");
    CHECK(arpa_load_words(nullptr, kVocab, kNVocab, 0, &m, &err) == kArpaErrArg, "null path");
  }
  fprintf(stderr, "fuzz corpus: %d files\n", n);
  if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
  printf("arpa_words_fuzz ok\n");
  return 0;
}
