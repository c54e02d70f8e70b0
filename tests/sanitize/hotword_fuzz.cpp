// CPU sanitizer pass over the hotword bank: built by tests/test_sanitize_hotword_cpu.py as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/sanitize/hotword_fuzz.cpp
// against lightning_asr_amd/csrc/hotword_io.h - the SAME source liblasr.so compiles (ctc_beam.hip wraps it, and its search
// kernels call the same walker).  No GPU, no HIP.
// Exit code 0 = every case behaved (a clean error or a consistent image and walk); any sanitizer report aborts with a non-zero code.
//
//   1. a hand-made bank builds, its image is self-consistent (offsets inside the image, every child, fail and probe chain
//      stays inside it, credit / keep / flags agree with the trie) and the walk gives the hand-worked bonuses;
//   2. 2 000 LCG-driven banks (nested phrases, duplicates, 32-label phrases, large label ids) x label sequences: build, write
//      image, walk - the bonus is the sum of the deltas, final never exceeds it, the state is a node;
//   3. hostile arguments: null pointers, labels outside [0, C) or equal to the blank, empty and over-long phrases, offsets that
//      run backwards, non-finite and non-positive weights, too many phrases, too many nodes: each fails with a message;
//   4. damaged images (every truncation of a good one, 3 000 byte mutations): hotword_score either rejects the image or walks
//      it without leaving it.
#include "../../lightning_asr_amd/csrc/hotword_io.h"

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

static uint64_t g_lcg = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33) % n;
}

struct Phrases {
  std::vector<int32_t> labels;
  std::vector<int64_t> offsets{0};
  std::vector<float> weights;
  void add(const std::vector<int32_t>& p, float w) {
    labels.insert(labels.end(), p.begin(), p.end());
    offsets.push_back((int64_t)labels.size());
    weights.push_back(w);
  }
  int64_t n() const { return (int64_t)weights.size(); }
};

static int build(const Phrases& p, int64_t C, int64_t blank, HotwordBank* b, std::string* err) {
  return hotword_build(p.labels.data(), p.offsets.data(), p.weights.data(), p.n(), C, blank, b, err);
}

// the image's internal consistency: what the kernels rely on before they read it
static void check_image(const HotwordBank& b, int64_t C, int64_t blank, const char* what) {
  CHECK(b.image.size() >= sizeof(HotwordImageHeader), "%s: image too small", what);
  if (b.image.size() < sizeof(HotwordImageHeader)) return;
  HotwordImageHeader h;
  memcpy(&h, b.image.data(), sizeof(h));
  const size_t n_slots = (size_t)1 << h.log2_slots;
  CHECK(h.magic == kHotwordImageMagic && h.n_nodes >= 1 && (int64_t)h.n_nodes == b.n_nodes && (int64_t)h.n_phrases == b.n_phrases,
        "%s: header", what);
  CHECK(h.node_off == sizeof(h) && h.edge_off == h.node_off + (size_t)h.n_nodes * sizeof(HotwordNode) &&
            h.edge_off + n_slots * sizeof(HotwordEdge) == b.image.size() && h.image_bytes == b.image.size(), "%s: offsets", what);
  CHECK(h.n_classes == (uint32_t)C && h.blank == (uint32_t)blank && h.max_credit == b.max_credit, "%s: classes", what);
  const HotwordView m = hotword_open(b.image.data(), b.image.size());
  CHECK(m.ok, "%s: hotword_open", what);
  if (!m.ok) return;
  std::vector<int> parent(h.n_nodes, -1), nchild(h.n_nodes, 0);
  size_t used = 0;
  for (size_t i = 0; i < n_slots; ++i) {
    if (m.edge[i].key == kHotwordEmptyKey) continue;
    ++used;
    const uint64_t v = m.edge[i].key >> 32, c = m.edge[i].key & 0xffffffffu;
    CHECK(v < h.n_nodes && (int64_t)c < C && (int64_t)c != blank, "%s: key", what);
    CHECK(m.edge[i].child >= 1 && (uint32_t)m.edge[i].child < h.n_nodes, "%s: child", what);
    if (v < h.n_nodes && m.edge[i].child >= 1 && (uint32_t)m.edge[i].child < h.n_nodes) {
      CHECK(parent[m.edge[i].child] == -1, "%s: a node with two parents", what);
      parent[m.edge[i].child] = (int)v;
      ++nchild[v];
      CHECK(hotword_child(m, (int)v, (int)c) == m.edge[i].child, "%s: probe", what);
    }
  }
  CHECK(used + 1 == h.n_nodes && 2 * used <= n_slots, "%s: edges / load factor", what);
  float max_credit = 0.f;
  for (uint32_t v = 0; v < h.n_nodes; ++v) {
    const HotwordNode& nd = m.node[v];
    const uint32_t depth = nd.flags >> kHotwordDepthShift;
    CHECK(nd.fail >= 0 && (uint32_t)nd.fail < h.n_nodes, "%s: fail", what);
    if (v == 0) { CHECK(nd.fail == 0 && nd.credit == 0.f && nd.keep == 0.f && nd.flags == 0, "%s: root", what); continue; }
    CHECK(parent[v] >= 0 && depth >= 1 && depth <= (uint32_t)kHotwordMaxLen, "%s: depth", what);
    if (parent[v] < 0) continue;
    const HotwordNode& pd = m.node[parent[v]];
    CHECK(depth == (pd.flags >> kHotwordDepthShift) + 1, "%s: depth chain", what);
    CHECK((m.node[nd.fail].flags >> kHotwordDepthShift) < depth, "%s: fail is a shorter string", what);
    CHECK(nd.credit > 0.f && nd.credit <= b.max_credit, "%s: credit", what);
    CHECK(nd.keep == ((nd.flags & kHotwordEnd) ? nd.credit : pd.keep), "%s: keep", what);
    CHECK(((nd.flags & kHotwordLeaf) != 0) == ((nd.flags & kHotwordEnd) && nchild[v] == 0), "%s: leaf", what);
    CHECK(nchild[v] > 0 || (nd.flags & kHotwordEnd), "%s: a childless node ends a phrase", what);
    if (nd.credit > max_credit) max_credit = nd.credit;
  }
  CHECK(max_credit == b.max_credit, "%s: max_credit", what);
}

// walks seq label by label: bonus(n) = bonus(n-1) + a finite delta, final <= bonus + 0 only through the give-back, state a node
static void check_walk(const HotwordBank& b, const std::vector<int32_t>& seq, const char* what) {
  std::string err;
  float prev = 0.f;
  for (size_t n = 0; n <= seq.size(); ++n) {
    float bonus = -1.f, fin = -1.f;
    int32_t st = -1;
    const int rc = hotword_score(b.image.data(), b.image.size(), seq.data(), (int64_t)n, &bonus, &fin, &st, &err);
    CHECK(rc == kHotwordOk, "%s: walk of %zu labels: %s", what, n, err.c_str());
    if (rc != kHotwordOk) return;
    CHECK(st >= 0 && st < b.n_nodes && std::isfinite(bonus) && std::isfinite(fin), "%s: walk result", what);
    CHECK(n > 0 || (bonus == 0.f && fin == 0.f && st == 0), "%s: the empty prefix", what);
    CHECK(st != 0 || fin == bonus, "%s: at the root nothing is given back", what);
    CHECK(std::fabs(bonus - prev) <= 2.f * b.max_credit + 1e-3f, "%s: one step moved the bonus by more than two credits", what);
    prev = bonus;
  }
}

int main(int argc, char** argv) {
  (void)argc; (void)argv;
  std::string err;
  int n_banks = 0;
  {  // 1. the hand-made bank: "ab" (w 2) inside "abc" (w 1), "bcd" (w 1.5), "e" (w 4)
    Phrases p;
    p.add({1, 2, 3}, 1.f); p.add({1, 2}, 2.f); p.add({2, 3, 4}, 1.5f); p.add({5}, 4.f);
    HotwordBank b;
    CHECK(build(p, 28, 27, &b, &err) == kHotwordOk, "hand-made bank: %s", err.c_str());
    CHECK(b.n_phrases == 4 && b.n_nodes == 8 && b.max_credit == 4.5f, "hand-made bank: counts");
    check_image(b, 28, 27, "hand-made");
    const std::vector<int32_t> seq = {1, 2, 3, 4, 5, 1, 2, 9, 1};
    const float want_b[] = {0, 2, 4, 3, 3, 7, 9, 11, 11, 13}, want_f[] = {0, 0, 4, 3, 3, 7, 7, 11, 11, 11};
    for (size_t n = 0; n <= seq.size(); ++n) {
      float bonus, fin;
      int32_t st;
      CHECK(hotword_score(b.image.data(), b.image.size(), seq.data(), (int64_t)n, &bonus, &fin, &st, &err) == kHotwordOk, "hand walk");
      CHECK(bonus == want_b[n] && fin == want_f[n], "hand walk at %zu: %g %g", n, bonus, fin);
    }
    check_walk(b, seq, "hand-made");
    HotwordBank e;   // the empty bank
    CHECK(hotword_build(nullptr, nullptr, nullptr, 0, 28, 27, &e, &err) == kHotwordOk && e.n_nodes == 1 && e.max_credit == 0.f, "empty bank");
    check_image(e, 28, 27, "empty");
    check_walk(e, seq, "empty");
    n_banks += 2;
  }
  // 2. random banks
  for (int it = 0; it < 2000; ++it) {
    const int64_t C = it % 3 == 0 ? 4334 : it % 3 == 1 ? 28 : 7;
    const int64_t blank = it % 5 == 0 ? 0 : C - 1;
    const uint32_t spread = it % 4 == 0 ? (uint32_t)C : 5;          // few labels: phrases overlap
    auto label = [&]() { int32_t c; do { c = (int32_t)rnd(spread); } while (c == blank); return c; };
    Phrases p;
    const int n = 1 + (int)rnd(it % 50 == 0 ? 600 : 12);
    std::vector<std::vector<int32_t>> all;
    for (int i = 0; i < n; ++i) {
      std::vector<int32_t> ph;
      const uint32_t kind = rnd(5);
      if (!all.empty() && kind == 0) {                               // a prefix of an earlier phrase, or the phrase again
        ph = all[rnd((uint32_t)all.size())];
        ph.resize(1 + rnd((uint32_t)ph.size()));
      } else if (!all.empty() && kind == 1) {                        // an earlier phrase's tail, extended
        const std::vector<int32_t>& q = all[rnd((uint32_t)all.size())];
        ph.assign(q.begin() + (q.size() > 2 ? q.size() - 2 : 0), q.end());
        for (uint32_t k = rnd(3); k > 0; --k) ph.push_back(label());
      } else {
        const int len = it % 7 == 0 ? kHotwordMaxLen : 1 + (int)rnd(6);
        for (int k = 0; k < len; ++k) ph.push_back(label());
      }
      if ((int)ph.size() > kHotwordMaxLen) ph.resize(kHotwordMaxLen);
      all.push_back(ph);
      p.add(ph, 0.25f * (float)(1 + rnd(40)));
    }
    HotwordBank b;
    const int rc = build(p, C, blank, &b, &err);
    CHECK(rc == kHotwordOk, "random bank %d: %s", it, err.c_str());
    if (rc != kHotwordOk) continue;
    check_image(b, C, blank, "random");
    std::vector<unsigned char> copy(b.image.size());                 // "write image": the walk runs on a copy elsewhere in memory
    memcpy(copy.data(), b.image.data(), copy.size());
    HotwordBank moved = b;
    moved.image.swap(copy);
    for (int s = 0; s < 3; ++s) {
      std::vector<int32_t> seq;
      for (uint32_t parts = 1 + rnd(8); parts > 0; --parts) {
        const uint32_t kind = rnd(3);
        const std::vector<int32_t>& q = all[rnd((uint32_t)all.size())];
        if (kind == 0) seq.insert(seq.end(), q.begin(), q.end());
        else if (kind == 1) seq.insert(seq.end(), q.begin(), q.begin() + 1 + rnd((uint32_t)q.size()));
        else seq.push_back(label());
      }
      check_walk(moved, seq, "random");
    }
    ++n_banks;
  }
  {  // 3. hostile arguments
    HotwordBank b;
    Phrases good;
    good.add({1, 2}, 1.f); good.add({3}, 2.f);
    auto expect = [&](const Phrases& p, int64_t C, int64_t blank, int want, const char* what) {
      err.clear();
      const int rc = build(p, C, blank, &b, &err);
      CHECK(rc == want && !err.empty(), "%s: rc %d (%s)", what, rc, err.c_str());
    };
    CHECK(hotword_build(nullptr, good.offsets.data(), good.weights.data(), 2, 28, 27, &b, &err) == kHotwordErrArg, "null labels");
    CHECK(hotword_build(good.labels.data(), nullptr, good.weights.data(), 2, 28, 27, &b, &err) == kHotwordErrArg, "null offsets");
    CHECK(hotword_build(good.labels.data(), good.offsets.data(), nullptr, 2, 28, 27, &b, &err) == kHotwordErrArg, "null weights");
    CHECK(hotword_build(good.labels.data(), good.offsets.data(), good.weights.data(), 2, 28, 27, nullptr, &err) == kHotwordErrArg, "null bank");
    CHECK(hotword_build(good.labels.data(), good.offsets.data(), good.weights.data(), -1, 28, 27, &b, &err) == kHotwordErrArg, "negative n");
    expect(good, 0, 0, kHotwordErrArg, "C = 0");
    expect(good, 28, 28, kHotwordErrArg, "blank = C");
    expect(good, 28, -1, kHotwordErrArg, "blank < 0");
    expect(good, 3, 0, kHotwordErrArg, "label = C");
    expect(good, 28, 3, kHotwordErrArg, "label = blank");
    { Phrases p = good; p.labels[0] = -5; expect(p, 28, 27, kHotwordErrArg, "negative label"); }
    { Phrases p = good; p.labels[0] = 0x7fffffff; expect(p, 28, 27, kHotwordErrArg, "huge label"); }
    { Phrases p = good; p.offsets[1] = 0; expect(p, 28, 27, kHotwordErrArg, "empty phrase"); }
    { Phrases p = good; p.offsets[1] = 3; p.offsets[2] = 2; expect(p, 28, 27, kHotwordErrArg, "offsets run backwards"); }
    { Phrases p = good; p.offsets[0] = -1; expect(p, 28, 27, kHotwordErrArg, "negative offset"); }
    { Phrases p; p.add(std::vector<int32_t>(kHotwordMaxLen + 1, 1), 1.f); expect(p, 28, 27, kHotwordErrArg, "over-long phrase"); }
    const float bad_w[] = {0.f, -1.f, INFINITY, -INFINITY, NAN};
    for (float w : bad_w) { Phrases p = good; p.weights[1] = w; expect(p, 28, 27, kHotwordErrArg, "bad weight"); }
    { Phrases p; for (int i = 0; i <= kHotwordMaxPhrases; ++i) p.add({1}, 1.f); expect(p, 28, 27, kHotwordErrFormat, "too many phrases"); }
    { Phrases p;                                                     // 40 000 phrases of 32 distinct-ish labels: over 2^20 nodes
      for (int i = 0; i < 40000; ++i) { std::vector<int32_t> ph; for (int k = 0; k < kHotwordMaxLen; ++k) ph.push_back((int32_t)rnd(4000)); p.add(ph, 1.f); }
      expect(p, 4334, 4333, kHotwordErrFormat, "too many nodes"); }
    float x;
    int32_t st;
    CHECK(hotword_score(nullptr, 64, nullptr, 0, &x, &x, &st, &err) == kHotwordErrArg, "score: null image");
  }
  int n_damaged = 0;
  {  // 4. damaged images
    Phrases p;
    p.add({1, 2, 3}, 1.f); p.add({1, 2}, 2.f); p.add({2, 3, 4}, 1.5f); p.add({5}, 4.f); p.add({3, 1, 2, 3, 4}, 0.5f);
    HotwordBank b;
    CHECK(build(p, 28, 27, &b, &err) == kHotwordOk, "bank to damage");
    const std::vector<int32_t> seq = {1, 2, 3, 1, 2, 3, 4, 5, 2, 3, 1, 2, 9, 3, 1, 2, 3, 4};
    float bonus, fin;
    int32_t st;
    for (size_t cut = 0; cut < b.image.size(); ++cut) {              // every truncation: rejected (the header says how long it is)
      std::vector<unsigned char> t(b.image.begin(), b.image.begin() + cut);
      const int rc = hotword_score(t.data(), t.size(), seq.data(), (int64_t)seq.size(), &bonus, &fin, &st, &err);
      CHECK(rc != kHotwordOk, "a %zu-byte truncation was walked", cut);
      ++n_damaged;
    }
    for (int it = 0; it < 3000; ++it) {                              // byte mutations: rejected, or walked inside the image
      std::vector<unsigned char> t = b.image;
      for (uint32_t k = 1 + rnd(4); k > 0; --k) t[rnd((uint32_t)t.size())] = (unsigned char)rnd(256);
      const int rc = hotword_score(t.data(), t.size(), seq.data(), (int64_t)seq.size(), &bonus, &fin, &st, &err);
      CHECK(rc == kHotwordOk || !err.empty(), "mutation %d: no message", it);
      if (rc == kHotwordOk) CHECK(st >= 0 && st < b.n_nodes, "mutation %d: state %d", it, st);
      ++n_damaged;
    }
  }
  fprintf(stderr, "fuzz corpus: %d banks, %d damaged images\n", n_banks, n_damaged);
  if (g_fail) { fprintf(stderr, "%d failures\n", g_fail); return 1; }
  printf("hotword_fuzz ok\n");
  return 0;
}
