// Hotword (phrase) biasing of the CTC beam search: the host-side builder of the biasing automaton, its device image and the
// one walker both sides call (ctc_beam.hip, lasr_hotword_* and lasr_ctc_beam_decode_bias / _lm_bias).  Plain C++17, no HIP
// header, so that the same source also builds as a g++ -fsanitize=address,undefined test binary
// (tests/sanitize/hotword_fuzz.cpp, run by tests/test_sanitize_hotword_cpu.py); under hipcc the walker is also a device function.
//
// A bank is n phrases of 1..kHotwordMaxLen label ids in [0, C), none the blank, each with a weight w > 0 (natural-log units per
// matched label).  Over the trie of the phrases every node v carries
//   depth(v); wmax(v) = the largest weight of a phrase through v; credit(v) = depth(v) * wmax(v) (f64, stored as f32; root 0);
//   end(v): a phrase ends at v; leaf(v): end(v) and v has no child;
//   keep(v) = credit of the deepest end node on the path root..v (v included), 0 if there is none;
//   fail(v) = the node of the longest proper suffix of v's string that is a trie node (the root if none; fail(root) = root).
// step(v, c) -> (v', delta):  v has a child u by c: delta = credit(u) - credit(v).  Otherwise w = fail(v); while w is not the
// root and has no child by c, w = fail(w); u = the child of w by c, or the root; delta = keep(v) - credit(v) + credit(u): the
// provisional credit beyond the last completed phrase is given back, the suffix match is credited.  v' = the root if leaf(u)
// (a completed phrase with no longer continuation is banked), else u.
// bonus(prefix) = the sum of the deltas from the root, state(prefix) = the node reached, final(prefix) = bonus + keep(state) -
// credit(state): all three depend on the prefix alone.
//
// Device image (one contiguous block, all offsets from its start, little-endian; read-only and position-independent):
//   HotwordImageHeader (64 bytes)
//   node[n_nodes]          HotwordNode (16 bytes): fail, credit, keep, flags (bit 0 end, bit 1 leaf, bits 8.. depth); node 0 = root
//   edge[1 << log2_slots]  HotwordEdge (16 bytes): open-addressing hash (linear probing, load <= 1/2) keyed exactly by
//                          (node << 32 | label) -> child.  The transition is sparse: no table over nodes x C exists.
#pragma once
#include <cmath>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define LASR_HOTWORD_HD __host__ __device__ __attribute__((always_inline))   // no call, no stack frame in the search kernels
#else
#define LASR_HOTWORD_HD
#endif

namespace lasr {
namespace host {

constexpr int kHotwordMaxLen = 32;
constexpr int64_t kHotwordMaxPhrases = 65536;
constexpr int64_t kHotwordMaxNodes = (int64_t)1 << 20;
constexpr uint32_t kHotwordImageMagic = 0x57485341u;   // "ASHW"
constexpr uint64_t kHotwordEmptyKey = ~0ull;
constexpr uint32_t kHotwordEnd = 1u, kHotwordLeaf = 2u;
constexpr int kHotwordDepthShift = 8;
constexpr uint32_t kHotwordMaxProbes = 64;              // the builder places every edge within this many slots of its home
constexpr int kHotwordRootUnknown = -2;                 // hotword_step's root_child when the caller has not resolved it
enum { kHotwordOk = 0, kHotwordErrArg = 1, kHotwordErrFormat = 2 };

struct HotwordImageHeader {
  uint32_t magic, n_nodes, n_phrases, log2_slots;
  float max_credit;
  uint32_t n_classes, blank, reserved0;
  uint64_t node_off, edge_off, image_bytes, reserved1;
};
static_assert(sizeof(HotwordImageHeader) == 64, "image header is 64 bytes");

struct alignas(16) HotwordNode {
  int32_t fail;
  float credit, keep;
  uint32_t flags;
};
static_assert(sizeof(HotwordNode) == 16, "one 16-byte load per node");

struct alignas(16) HotwordEdge {
  uint64_t key;                                          // node << 32 | label, kHotwordEmptyKey when free
  int32_t child, reserved;
};
static_assert(sizeof(HotwordEdge) == 16, "one 16-byte load per probe");

// an opened image: what the walker reads
struct HotwordView {
  const HotwordNode* node;
  const HotwordEdge* edge;
  uint32_t mask, n_nodes, n_classes, blank;
  float max_credit;
  bool ok;                                               // the header is a hotword image's
};

// the slot a key starts probing at (splitmix64's finaliser, as the LM image's hash)
LASR_HOTWORD_HD inline uint64_t hotword_hash(uint64_t k) {
  k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
  k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

// Opens an image for reading.  `bytes`: its size where the caller knows it (the host), 0 where it does not (the device, which
// trusts an image whose header is consistent).  !ok: nothing else of the view may be used.
LASR_HOTWORD_HD inline HotwordView hotword_open(const void* image, uint64_t bytes) {
  const HotwordImageHeader* h = static_cast<const HotwordImageHeader*>(image);
  const char* base = static_cast<const char*>(image);
  HotwordView m;
  m.ok = h->magic == kHotwordImageMagic && h->n_nodes >= 1 && (int64_t)h->n_nodes <= kHotwordMaxNodes && h->log2_slots >= 4 &&
         h->log2_slots < 32 && h->node_off == sizeof(HotwordImageHeader) &&
         h->edge_off == h->node_off + (uint64_t)h->n_nodes * sizeof(HotwordNode) &&
         h->image_bytes == h->edge_off + ((uint64_t)1 << h->log2_slots) * sizeof(HotwordEdge) &&
         (bytes == 0 || bytes >= h->image_bytes);
  m.node = reinterpret_cast<const HotwordNode*>(base + (m.ok ? h->node_off : 0));
  m.edge = reinterpret_cast<const HotwordEdge*>(base + (m.ok ? h->edge_off : 0));
  m.mask = m.ok ? (1u << h->log2_slots) - 1u : 0u;
  m.n_nodes = m.ok ? h->n_nodes : 0u;
  m.n_classes = h->n_classes;
  m.blank = h->blank;
  m.max_credit = m.ok ? h->max_credit : 0.f;
  return m;
}

LASR_HOTWORD_HD inline uint64_t hotword_key(int v, int c) { return ((uint64_t)(uint32_t)v << 32) | (uint32_t)c; }

// index of the slot (v, c) starts probing at.  A caller with several walks to make loads these slots together and hands each
// to hotword_step, so that the loads are in flight at once.
LASR_HOTWORD_HD inline uint32_t hotword_slot(const HotwordView& m, int v, int c) {
  return (uint32_t)hotword_hash(hotword_key(v, c)) & m.mask;
}

// the child of `key` = node << 32 | label, or -1; e = the slot at `at`, already loaded.  At most kHotwordMaxProbes slots are
// read: the builder places every edge that close to its home slot, so a longer run is a miss - and a damaged image whose table
// has no free slot costs a probe 64 loads, not a scan of the table.
LASR_HOTWORD_HD inline int hotword_child_rest(const HotwordView& m, uint64_t key, uint32_t at, HotwordEdge e) {
  for (uint32_t n = 0; n < kHotwordMaxProbes; ++n) {
    if (e.key == key) return (uint32_t)e.child < m.n_nodes ? e.child : -1;
    if (e.key == kHotwordEmptyKey) return -1;
    at = (at + 1) & m.mask;
    e = m.edge[at];
  }
  return -1;
}

LASR_HOTWORD_HD inline int hotword_child(const HotwordView& m, int v, int c) {
  const uint32_t at = hotword_slot(m, v, c);
  return hotword_child_rest(m, hotword_key(v, c), at, m.edge[at]);
}

// THE walker: one step of the automaton from node v by label c.  `first` = m.edge[hotword_slot(m, v, c)], loaded by the caller
// (not read when v is the root and root_child is known).  root_child = the root's child by c (hotword_child(m, 0, c): -1 if it
// has none), or kHotwordRootUnknown.  Returns v' and sets *delta.  Holds the probe, the fail loop (bounded by the depth) and
// the leaf reset.
LASR_HOTWORD_HD inline int hotword_step(const HotwordView& m, int v, int c, int root_child, HotwordEdge first, float* delta) {
  // one loop down the fail chain from w = v: the first pass is the child match, the pass at the root ends the chain
  int u = -1, w = v;
  for (int i = 0; i <= kHotwordMaxLen + 1; ++i) {
    if (w == 0 && root_child != kHotwordRootUnknown) { u = root_child; break; }
    const uint32_t at = hotword_slot(m, w, c);
    u = hotword_child_rest(m, hotword_key(w, c), at, i == 0 ? first : m.edge[at]);
    if (u >= 0 || w == 0) break;
    w = m.node[w].fail;
    if ((uint32_t)w >= m.n_nodes) w = 0;                   // a node id the image does not hold reads as the root
  }
  const bool matched = u >= 0 && w == v;                   // v has the child u
  if (u < 0) u = 0;
  const HotwordNode nu = m.node[u];
  float d = nu.credit;                                     // from the root: keep(root) = credit(root) = 0
  if (v != 0) {
    const HotwordNode nv = m.node[v];
    d = matched ? nu.credit - nv.credit : (nv.keep - nv.credit) + nu.credit;
  }
  *delta = d;
  return (nu.flags & kHotwordLeaf) ? 0 : u;
}

// final(prefix) - bonus(prefix) for a prefix in state v: an unfinished match gives its provisional credit back
LASR_HOTWORD_HD inline float hotword_give_back(const HotwordView& m, int v) {
  if (v == 0) return 0.f;
  const HotwordNode nv = m.node[v];
  return nv.keep - nv.credit;
}

struct HotwordBank {
  int64_t n_phrases = 0, n_nodes = 0;
  float max_credit = 0.f;
  std::vector<unsigned char> image;
};

// Builds the automaton and its image.  labels: the phrases back to back, phrase i = labels[offsets[i] .. offsets[i + 1]).
// kHotwordErrArg: a null pointer, a label outside [0, C) or equal to the blank, an empty or over-long phrase, a weight that is
// not finite and > 0; kHotwordErrFormat: too many phrases or trie nodes.  *err names the phrase.
static inline int hotword_build(const int32_t* labels, const int64_t* offsets, const float* weights, int64_t n_phrases, int64_t C,
                                int64_t blank, HotwordBank* out, std::string* err) {
  if (!out || !err) return kHotwordErrArg;
  if (n_phrases < 0) { *err = "negative phrase count"; return kHotwordErrArg; }
  if (n_phrases > 0 && (!labels || !offsets || !weights)) { *err = "null pointer"; return kHotwordErrArg; }
  if (C < 1 || C > 0x7fffffffLL || blank < 0 || blank >= C) {
    *err = "blank " + std::to_string((long long)blank) + " outside [0, C = " + std::to_string((long long)C) + ")";
    return kHotwordErrArg;
  }
  if (n_phrases > kHotwordMaxPhrases) {
    *err = std::to_string((long long)n_phrases) + " phrases: a bank holds at most " + std::to_string((long long)kHotwordMaxPhrases);
    return kHotwordErrFormat;
  }
  auto at_phrase = [](int64_t i, const std::string& what) { return "phrase " + std::to_string((long long)i) + ": " + what; };
  // every phrase is checked before the trie is built
  for (int64_t i = 0; i < n_phrases; ++i) {
    const int64_t a = offsets[i], b = offsets[i + 1];
    if (a < 0 || b < a) { *err = at_phrase(i, "offsets are not ascending from 0"); return kHotwordErrArg; }
    if (b == a) { *err = at_phrase(i, "empty"); return kHotwordErrArg; }
    if (b - a > kHotwordMaxLen) {
      *err = at_phrase(i, std::to_string((long long)(b - a)) + " labels: a phrase holds at most " + std::to_string(kHotwordMaxLen));
      return kHotwordErrArg;
    }
    if (!(std::isfinite(weights[i]) && weights[i] > 0.f)) { *err = at_phrase(i, "its weight is not finite and > 0"); return kHotwordErrArg; }
    for (int64_t j = a; j < b; ++j) {
      const int64_t c = labels[j];
      if (c < 0 || c >= C) {
        *err = at_phrase(i, "label " + std::to_string((long long)c) + " outside [0, " + std::to_string((long long)C) + ")");
        return kHotwordErrArg;
      }
      if (c == blank) { *err = at_phrase(i, "label " + std::to_string((long long)c) + " is the blank"); return kHotwordErrArg; }
    }
  }
  // the trie
  std::unordered_map<uint64_t, uint32_t> edge;
  std::vector<int32_t> parent(1, 0), label(1, -1), depth(1, 0), nchild(1, 0);
  std::vector<float> wmax(1, 0.f);
  std::vector<char> end(1, 0);
  for (int64_t i = 0; i < n_phrases; ++i) {
    uint32_t v = 0;
    for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
      const uint64_t key = hotword_key((int)v, labels[j]);
      auto it = edge.find(key);
      if (it == edge.end()) {
        if ((int64_t)parent.size() >= kHotwordMaxNodes) {
          *err = at_phrase(i, "the bank needs more than " + std::to_string((long long)kHotwordMaxNodes) + " trie nodes");
          return kHotwordErrFormat;
        }
        it = edge.emplace(key, (uint32_t)parent.size()).first;
        parent.push_back((int32_t)v);
        label.push_back(labels[j]);
        depth.push_back(depth[v] + 1);
        nchild.push_back(0);
        wmax.push_back(0.f);
        end.push_back(0);
        ++nchild[v];
      }
      v = it->second;
      if (weights[i] > wmax[v]) wmax[v] = weights[i];
    }
    end[v] = 1;
  }
  const size_t n_nodes = parent.size();
  // nodes by depth: a node's fail and keep need those of shallower nodes only
  std::vector<uint32_t> order(n_nodes);
  {
    std::vector<size_t> start(kHotwordMaxLen + 2, 0);
    for (size_t v = 0; v < n_nodes; ++v) ++start[depth[v] + 1];
    for (int d = 0; d <= kHotwordMaxLen; ++d) start[d + 1] += start[d];
    for (size_t v = 0; v < n_nodes; ++v) order[start[depth[v]]++] = (uint32_t)v;
  }
  std::vector<int32_t> fail(n_nodes, 0);
  std::vector<float> credit(n_nodes, 0.f), keep(n_nodes, 0.f);
  float max_credit = 0.f;
  for (size_t k = 1; k < n_nodes; ++k) {
    const uint32_t v = order[k];
    credit[v] = (float)((double)depth[v] * (double)wmax[v]);
    if (credit[v] > max_credit) max_credit = credit[v];
    keep[v] = end[v] ? credit[v] : keep[parent[v]];
    if (depth[v] > 1) {
      int32_t w = fail[parent[v]];
      while (true) {
        auto it = edge.find(hotword_key(w, label[v]));
        if (it != edge.end()) { fail[v] = (int32_t)it->second; break; }
        if (w == 0) break;
        w = fail[w];
      }
    }
  }
  // the table: load <= 1/2, doubled until every edge sits within kHotwordMaxProbes slots of its home (at that load a longer
  // run is vanishingly rare, but the walker's probe bound relies on there being none)
  int log2_slots = 4;
  while (((size_t)1 << log2_slots) < 2 * edge.size()) ++log2_slots;
  std::vector<unsigned char> img;
  HotwordImageHeader h;
  bool placed = false;
  for (;; ++log2_slots) {
    const size_t n_slots = (size_t)1 << log2_slots;
    memset(&h, 0, sizeof(h));
    h.magic = kHotwordImageMagic;
    h.n_nodes = (uint32_t)n_nodes;
    h.n_phrases = (uint32_t)n_phrases;
    h.log2_slots = (uint32_t)log2_slots;
    h.max_credit = max_credit;
    h.n_classes = (uint32_t)C;
    h.blank = (uint32_t)blank;
    h.node_off = sizeof(HotwordImageHeader);
    h.edge_off = h.node_off + n_nodes * sizeof(HotwordNode);
    h.image_bytes = h.edge_off + n_slots * sizeof(HotwordEdge);
    img.assign((size_t)h.image_bytes, 0);
    HotwordEdge* e = reinterpret_cast<HotwordEdge*>(img.data() + h.edge_off);
    for (size_t i = 0; i < n_slots; ++i) { e[i].key = kHotwordEmptyKey; e[i].child = -1; e[i].reserved = 0; }
    placed = true;
    // in node order, so that the image does not depend on the hash map's iteration order
    for (size_t v = 1; v < n_nodes && placed; ++v) {
      const uint64_t key = hotword_key(parent[v], label[v]);
      size_t at = (size_t)(hotword_hash(key) & (n_slots - 1));
      uint32_t far = 0;
      while (e[at].key != kHotwordEmptyKey && ++far < kHotwordMaxProbes) at = (at + 1) & (n_slots - 1);
      if (e[at].key != kHotwordEmptyKey) { placed = false; break; }
      e[at].key = key;
      e[at].child = (int32_t)v;
    }
    if (placed || log2_slots >= 30) break;
  }
  if (!placed) { *err = "the edge table cannot be built"; return kHotwordErrFormat; }
  memcpy(img.data(), &h, sizeof(h));
  HotwordNode* nd = reinterpret_cast<HotwordNode*>(img.data() + h.node_off);
  for (size_t v = 0; v < n_nodes; ++v) {
    nd[v].fail = fail[v];
    nd[v].credit = credit[v];
    nd[v].keep = keep[v];
    nd[v].flags = (end[v] ? kHotwordEnd : 0u) | (end[v] && nchild[v] == 0 ? kHotwordLeaf : 0u) |
                  ((uint32_t)depth[v] << kHotwordDepthShift);
  }
  out->n_phrases = n_phrases;
  out->n_nodes = (int64_t)n_nodes;
  out->max_credit = max_credit;
  out->image.swap(img);
  return kHotwordOk;
}

// The host walk of labels[0 .. n) over an image of `bytes` bytes: bonus, final and state of that prefix.  A label outside the
// image's classes, or its blank, is an argument error; so is an image hotword_open rejects.
static inline int hotword_score(const void* image, size_t bytes, const int32_t* labels, int64_t n, float* bonus, float* final_bonus,
                                int32_t* state, std::string* err) {
  if (!image || bytes < sizeof(HotwordImageHeader) || (n > 0 && !labels) || n < 0) { *err = "null pointer or negative length"; return kHotwordErrArg; }
  const HotwordView m = hotword_open(image, bytes);
  if (!m.ok) { *err = "not a hotword image"; return kHotwordErrFormat; }
  int v = 0;
  float b = 0.f;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t c = labels[i];
    if (c < 0 || (uint32_t)c >= m.n_classes || (uint32_t)c == m.blank) {
      *err = "label " + std::to_string(c) + " at position " + std::to_string((long long)i) + " is the blank or outside the bank's classes";
      return kHotwordErrArg;
    }
    float d;
    v = hotword_step(m, v, c, kHotwordRootUnknown, m.edge[hotword_slot(m, v, c)], &d);
    b += d;
  }
  if (bonus) *bonus = b;
  if (final_bonus) *final_bonus = b + hotword_give_back(m, v);
  if (state) *state = v;
  return kHotwordOk;
}

}  // namespace host
}  // namespace lasr
