// CTC prefix beam search: ctc_decoders' ctc_beam_search_decoder as used by the reference's BeamSearchDecoderWithLM
// (beam_search.py:17-57), without a scorer, with a character or a word n-gram LM, with hotword biasing, or with the character
// LM and hotwords together (include/lasr.h states each contract).  Blank is an argument (C-1 in this project).
//
// Two launches, no host synchronisation, no allocation:
//   1. beam_prune_kernel: one wave per (utterance, frame).  Ranks the classes by (log-prob desc, id asc) with a radix select
//      of the cutoff_top_n best (a direct 64-lane rank for C <= 64), applies cutoff_prob to the cumulative probability of
//      that run and writes the kept (class, log-prob) list of the frame into the workspace.
//   2. beam_search_kernel<J, Scorer>: one 256-thread workgroup per utterance, looping over its frames.  The beam (trie node,
//      last label, length, prefix hash, ACOUSTIC log_b / log_nb) lives in LDS; the frame's candidates (one "no new label" entry
//      per live prefix + one extension per (prefix, kept label)) live in registers, J per thread.  The beam_width best are
//      found by an 8-bit radix select over (score, tie-break key) that stops as soon as the boundary bucket is taken whole;
//      only the survivors are ordered (rank by counting).  New prefixes are appended to a parent-pointer trie in the workspace
//      (at most beam_width nodes per frame) that is walked back once at the end.
//
// There is one frame loop, beam_search_kernel, over the beam_* phases on BeamCore; what a search adds to the acoustic score is
// a Scorer policy: NullScorer, LmScorer<false / true> (character LM, without / with hotwords), BiasScorer (hotwords) and
// WlmScorer (word LM and lexicon).  A new scorer provides: Args (its kernel arguments) and Lds (BeamCore first, its
// per-survivor array right behind); open() (false: wrong image, every slot comes back empty); init_root() and begin_frame();
// prefix_bonus() / prefix_extras(), what core.score holds beyond logaddexp(b, nb); kCutoff with logp / cut_slack for the early
// cutoff; Group with clear / issue / chain / finish, the scoring of kLmGroup extensions whose probes are in flight together,
// and the Carry a survivor takes through beam_compact (on_keep); keep_entry() / new_entry() for its per-entry fields;
// final_scores() with kOuts, kRerank, fin() and extra_out() for the end of the utterance.  The body never re-associates the
// sums a scorer returns: the parenthesisation of every score is part of the result.
//
// Prefix identity: p+c merges with a live entry q when q's parent prefix equals p and q's last label is c.  Entries carry a
// 64-bit hash of their label sequence and of their parent's, so "q's parent equals p" is a hash compare; a trie node id
// would not do, since a prefix that left the beam and came back gets a new node while its children may still be live.
#include <type_traits>

#include "common.h"
#include "arpa_io.h"
#include "hotword_io.h"

namespace lasr {
namespace {

constexpr int kBeamMaxWidth = 128;
constexpr int kBeamMaxTopN = 64;
constexpr int kBeamMaxClasses = 8192;
constexpr int kSearchThreads = 256;
constexpr float kNegInfB = -INFINITY;
constexpr uint64_t kRootHash = 0x6a09e667f3bcc908ull;

__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == kNegInfB) return m;
  return m + log1pf(expf(fminf(a, b) - m));
}

// ascending in the result == descending in f (f is never NaN here; -0 is folded onto +0 first)
__device__ __forceinline__ uint32_t desc_bits(float f) {
  uint32_t u = __float_as_uint(f + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

__device__ __forceinline__ uint64_t child_hash(uint64_t h, int c) {
  uint64_t z = h + 0x9e3779b97f4a7c15ull * (uint64_t)(c + 1);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// hist[bin] += 1 for every lane with `on`, one LDS atomic per distinct bin of the wave (the early radix digits of a frame's
// scores fall into a handful of bins, which plain per-lane atomics would serialise on)
__device__ __forceinline__ void wave_hist_add(uint32_t* hist, bool on, uint32_t bin, int lane) {
  bool pend = on;
  uint64_t act = __ballot(pend);
  while (act) {
    const int leader = __builtin_ctzll(act);
    const uint32_t lb = (uint32_t)__shfl((int)bin, leader, 64);
    const uint64_t same = __ballot(pend && bin == lb);
    if (lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
    pend = pend && bin != lb;
    act &= ~same;
  }
}

// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// One wave reads the 256-bin histogram (4 bins per lane), finds the bucket holding the need-th smallest element and zeroes
// the bins for the next pass.  out[0] = bucket, out[1] = elements in smaller buckets, out[2] = elements in the bucket,
// out[3] = total.
__device__ __forceinline__ void wave_find_bucket(uint32_t* hist, uint32_t need, int lane, uint32_t* out) {
  uint32_t h[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = hist[lane * 4 + i];
    s += h[i];
  }
  const uint32_t incl = wave_incl_scan(s, lane);
  uint32_t excl = incl - s;
  if (excl < need && need <= incl) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (excl < need && need <= excl + h[i]) {
        out[0] = lane * 4 + i;
        out[1] = excl;
        out[2] = h[i];
      }
      excl += h[i];
    }
  }
  if (lane == 63) out[3] = incl;
#pragma unroll
  for (int i = 0; i < 4; ++i) hist[lane * 4 + i] = 0;
}

// ------------------------------------------------------------------ frame pruning ---------------------------------------
// composite of a class: (desc log-prob) << 13 | class id: unique, ascending == the (log-prob desc, id asc) order
__device__ __forceinline__ uint64_t class_key(float v, int c) { return ((uint64_t)desc_bits(v) << 13) | (uint64_t)c; }

__global__ __launch_bounds__(64) void beam_prune_kernel(const float* __restrict__ logp, const int32_t* __restrict__ lens,
                                                        int64_t T, int C, int topn, float cutoff_prob,
                                                        int32_t* __restrict__ kcls, float* __restrict__ klp,
                                                        int32_t* __restrict__ kn) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t found[4];
  __shared__ uint64_t sel[kBeamMaxTopN];
  __shared__ uint32_t nsel;
  const int lane = threadIdx.x;
  const int64_t frame = blockIdx.x;
  const int64_t b = frame / T, t = frame - b * T;
  const int64_t L = lens ? min((int64_t)max(lens[b], 0), T) : T;
  if (t >= L) return;
  const float* row = logp + frame * (int64_t)C;
  const int K = min(topn, C);
  uint64_t mine = ~0ull;  // lane < K: the lane-th best composite once sorted
  if (C <= 64) {
    const uint64_t key = lane < C ? class_key(row[lane], lane) : ~0ull;
    int rank = 0;
    for (int j = 0; j < C; ++j) rank += (uint64_t)__shfl((long long)key, j, 64) < key;
    if (lane < C && rank < K) sel[rank] = key;
    __syncthreads();
    if (lane < K) mine = sel[lane];
  } else {
    // radix select of the K smallest composites (45 bits: 8-bit digits aligned to the f32 key, the last one overlapping)
    for (int i = lane; i < 256; i += 64) hist[i] = 0;
    if (lane == 0) nsel = 0;
    __syncthreads();
    uint64_t prefix = 0, mask = 0;
    uint32_t need = (uint32_t)K;
    for (int ps = 0; ps < 6; ++ps) {
      const int sh = ps < 5 ? 37 - 8 * ps : 0;
      for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        const uint64_t key = c < C ? class_key(row[c], c) : 0;
        wave_hist_add(hist, c < C && (key & mask) == prefix, (uint32_t)(key >> sh) & 255u, lane);
      }
      __syncthreads();
      wave_find_bucket(hist, need, lane, found);
      __syncthreads();
      const uint32_t bucket = found[0], before = found[1], cnt = found[2];
      prefix |= (uint64_t)bucket << sh;
      mask |= 0xffull << sh;
      need -= before;
      if (cnt == need) break;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int c = c0 + lane;
      const uint64_t key = c < C ? class_key(row[c], c) : ~0ull;
      if (c < C && (key & mask) <= prefix) {
        const uint32_t pos = atomicAdd(&nsel, 1u);
        if (pos < (uint32_t)kBeamMaxTopN) sel[pos] = key;   // exactly K land here; the guard only bounds the LDS index
      }
    }
    __syncthreads();
    uint64_t key = lane < K ? sel[lane] : ~0ull;
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += (uint64_t)__shfl((long long)key, j, 64) < key;
    __syncthreads();
    if (lane < K) sel[rank] = key;
    __syncthreads();
    if (lane < K) mine = sel[lane];
  }
  const int cls = (int)(mine & 8191u);
  const float v = lane < K ? row[cls] : kNegInfB;
  int keep = K;
  if (cutoff_prob < 1.0f) {
    // shortest leading run whose cumulative probability reaches cutoff_prob
    float cum = lane < K ? expf(v) : 0.f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float u = __shfl_up(cum, o, 64);
      if (lane >= o) cum += u;
    }
    const uint64_t reached = __ballot(lane < K && cum >= cutoff_prob);
    if (reached) keep = min(K, __builtin_ctzll(reached) + 1);
  }
  if (lane < keep) {
    kcls[frame * kBeamMaxTopN + lane] = cls;
    klp[frame * kBeamMaxTopN + lane] = v;
  }
  if (lane == 0) kn[frame] = keep;
}

// ------------------------------------------------------------------ the search: phases ----------------------------------
// What every search keeps in LDS.  The phases below (beam_init_root .. beam_write_back) work on this alone; b / nb are always
// ACOUSTIC, score is what the beam is ranked by.
struct BeamCore {
  int node[2][kBeamMaxWidth], last[2][kBeamMaxWidth], len[2][kBeamMaxWidth];
  float b[2][kBeamMaxWidth], nb[2][kBeamMaxWidth];       // acoustic log_b / log_nb
  uint64_t h[2][kBeamMaxWidth], ph[2][kBeamMaxWidth];
  float score[kBeamMaxWidth];             // what the current beam is ranked by: logaddexp(b, nb) (+ the scorer's bonus, if any)
  float next_b[kBeamMaxWidth], next_nb[kBeamMaxWidth];   // the "no new label" candidate of each live prefix
  unsigned long long merged[kBeamMaxWidth];              // bit k: p + kept[k] merged into a live entry
  uint64_t surv[kBeamMaxWidth];
  int kcls[kBeamMaxTopN];
  float klp[kBeamMaxTopN];
  uint32_t hist[256];
  uint32_t found[4];
  uint32_t nsel;
  // last, and aligned so that the struct has no tail padding: a per-survivor array that a scorer places right behind its
  // BeamCore is then 512 bytes from surv_i, and beam_compact's store and on_keep's go out as one paired LDS write
  alignas(8) int surv_i[kBeamMaxWidth];
};

// the root entry (the empty prefix) and a zeroed histogram; the first frame's barrier publishes them
__device__ __forceinline__ void beam_init_root(BeamCore& s, int tid) {
  if (tid == 0) {
    s.node[0][0] = 0; s.last[0][0] = -1; s.len[0][0] = 0;
    s.b[0][0] = 0.f; s.nb[0][0] = kNegInfB;
    s.h[0][0] = kRootHash; s.ph[0][0] = 0;
  }
  for (int i = tid; i < 256; i += kSearchThreads) s.hist[i] = 0;
}

// The kept list of frame t + 1 is fetched into registers while frame t is searched.
struct BeamFetch {
  const int32_t* kc;    // this utterance's rows of the prune launch's output
  const float* kl;
  const int32_t* kn;
  int pc = 0, pn = 0;
  float pl = 0.f;
  __device__ __forceinline__ void request(int64_t t, int tid) {
    if (tid < kBeamMaxTopN) { pc = kc[t * kBeamMaxTopN + tid]; pl = kl[t * kBeamMaxTopN + tid]; }
    pn = kn[t];
  }
};

// publishes the requested frame t into kcls / klp, requests frame t + 1 and resets the survivor count; returns the number of
// kept labels.  The caller's barrier follows.
__device__ __forceinline__ int beam_fetch_frame(BeamCore& s, BeamFetch& f, int64_t t, int64_t L, int tid) {
  const int nk = f.pn;
  if (tid < nk) { s.kcls[tid] = f.pc; s.klp[tid] = f.pl; }
  if (t + 1 < L) f.request(t + 1, tid);
  if (tid == 0) s.nsel = 0;
  return nk;
}

// (1) for the live prefix `tid`, whose last label is `last`: the kept index of that label, the blank's kept log-prob and the
// prefix's parent among the live entries (found by hash); clears its merged bits
__device__ __forceinline__ void beam_lookup(BeamCore& s, int cur, int nbeam, int nk, int blank, int tid, int last, int* lastk,
                                            int* pr, float* blp) {
  s.merged[tid] = 0ull;
  for (int k = 0; k < nk; ++k) {
    const int c = s.kcls[k];
    if (c == last) *lastk = k;
    if (c == blank) *blp = s.klp[k];
  }
  if (last >= 0) {
    const uint64_t ph = s.ph[cur][tid];
    for (int r = 0; r < nbeam; ++r)
      if (s.h[cur][r] == ph) { *pr = r; break; }
  }
}

// (4) radix select of the W smallest composites among a thread's J (bit j of `valid`: comp[j] is finite); `prefix`/`mask`
// end as the boundary: (comp & mask) <= prefix is taken
template <int J>
__device__ __forceinline__ void beam_select(BeamCore& s, const uint64_t (&comp)[J], uint64_t valid, int W, int tid,
                                            uint64_t* prefix_out, uint64_t* mask_out) {
  const int lane = tid & 63;
  uint64_t prefix = 0, mask = 0;
  uint32_t need = (uint32_t)W;
#pragma nounroll
  for (int ps = 0; ps < 7; ++ps) {
    const int sh = ps < 4 ? 56 - 8 * ps : 16 - 8 * (ps - 4);   // the key is below 2^21: bits 21..31 are always 0
#pragma unroll
    for (int j = 0; j < J; ++j)
      wave_hist_add(s.hist, ((valid >> j) & 1ull) && (comp[j] & mask) == prefix, (uint32_t)(comp[j] >> sh) & 255u, lane);
    __syncthreads();
    if (tid < 64) wave_find_bucket(s.hist, need, lane, s.found);
    __syncthreads();
    if (ps == 0 && s.found[3] <= need) break;        // no more finite candidates than the beam holds: take them all
    const uint32_t bucket = s.found[0], before = s.found[1], cnt = s.found[2];
    prefix |= (uint64_t)bucket << sh;
    mask |= 0xffull << sh;
    need -= before;
    if (cnt == need) break;
  }
  *prefix_out = prefix;
  *mask_out = mask;
}

// (5), first half: compacts the survivors into surv / surv_i and returns their number once every thread's are in;
// on_keep(pos, j) lets the caller store more of candidate j at the same slot
template <int J, class OnKeep>
__device__ __forceinline__ int beam_compact(BeamCore& s, const uint64_t (&comp)[J], uint64_t valid, uint64_t prefix,
                                            uint64_t mask, int W, int tid, OnKeep on_keep) {
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (((valid >> j) & 1ull) && (comp[j] & mask) <= prefix) {
      const uint32_t pos = atomicAdd(&s.nsel, 1u);
      if (pos < (uint32_t)kBeamMaxWidth) {   // at most W survive; the guard only bounds the LDS index
        s.surv[pos] = comp[j];
        s.surv_i[pos] = tid + j * kSearchThreads;
        on_keep(pos, j);
      }
    }
  }
  __syncthreads();
  return min((int)s.nsel, W);
}

// (5), second half: only the survivors are ordered, by counting; the next beam is written in rank order
__device__ __forceinline__ int beam_rank(const BeamCore& s, int nsel, int tid) {
  const uint64_t me = s.surv[tid];
  int rank = 0;
  for (int r = 0; r < nsel; ++r) rank += s.surv[r] < me;
  return rank;
}

// entry i of the current beam survives without a new label
__device__ __forceinline__ void beam_keep_entry(BeamCore& s, int cur, int nxt, int rank, int i) {
  s.node[nxt][rank] = s.node[cur][i]; s.last[nxt][rank] = s.last[cur][i]; s.len[nxt][rank] = s.len[cur][i];
  s.h[nxt][rank] = s.h[cur][i]; s.ph[nxt][rank] = s.ph[cur][i];
  s.b[nxt][rank] = s.next_b[i]; s.nb[nxt][rank] = s.next_nb[i];
}

// entry p extended by label c survives as a new prefix: a trie node of frame t and an entry whose log_nb, the extension's
// acoustic score, the caller writes
__device__ __forceinline__ void beam_new_entry(BeamCore& s, int cur, int nxt, int rank, int p, int c, int64_t t, int W,
                                               int2* trie) {
  const int node = 1 + (int)t * W + rank;
  trie[node] = make_int2(s.node[cur][p], c);
  s.node[nxt][rank] = node; s.last[nxt][rank] = c; s.len[nxt][rank] = s.len[cur][p] + 1;
  s.h[nxt][rank] = child_hash(s.h[cur][p], c); s.ph[nxt][rank] = s.h[cur][p];
  s.b[nxt][rank] = kNegInfB;
}

// End of utterance, for the scorers whose end term can change the order.  Thread tid < nbeam hands in its entry's N final
// values, out[0] the score; the entries are ranked by it, ties by their order before, and (node, len) and the values are
// written in the new order: node / len into the other half of the beam, which is returned for beam_write_back (whose barrier
// publishes fin).
template <int N>
__device__ __forceinline__ int beam_final_rerank(BeamCore& core, float (&fin)[N][kBeamMaxWidth], int cur, int nbeam, int tid,
                                                 const float (&out)[N]) {
  if (tid < nbeam) core.score[tid] = out[0];
  __syncthreads();
  const int dst = cur ^ 1;
  if (tid < nbeam) {
    const float f = out[0];
    int rank = 0;
    for (int r = 0; r < nbeam; ++r) {
      const float g = core.score[r];
      rank += g > f || (g == f && r < tid);
    }
    core.node[dst][rank] = core.node[cur][tid]; core.len[dst][rank] = core.len[cur][tid];
#pragma unroll
    for (int n = 0; n < N; ++n) fin[n][rank] = out[n];
  }
  return dst;
}

// walks the trie back from each of the n_best final entries (none of them when !valid_all) into tok, this utterance's
// (n_best, T) tokens, and writes the lengths; the slots past a hypothesis are -1, the length of an empty slot is -1
__device__ __forceinline__ void beam_write_back(const BeamCore& s, int cur, int nbeam, int n_best, int64_t T, const int2* trie,
                                                int32_t* tok, int32_t* n_tokens, bool valid_all, int tid) {
  __threadfence();
  __syncthreads();
  if (!valid_all) nbeam = 0;
  if (tid < n_best) {
    if (tid < nbeam) {
      const int n = s.len[cur][tid];
      n_tokens[tid] = n;
      int node = s.node[cur][tid];
      for (int pos = n - 1; pos >= 0; --pos) {
        const int2 e = trie[node];
        tok[(int64_t)tid * T + pos] = e.y;
        node = e.x;
      }
    } else {
      n_tokens[tid] = -1;
    }
  }
  for (int64_t idx = tid; idx < (int64_t)n_best * T; idx += kSearchThreads) {
    const int j = (int)(idx / T);
    const int64_t pos = idx - (int64_t)j * T;
    const int n = j < nbeam ? s.len[cur][j] : 0;
    if (pos >= n) tok[idx] = -1;
  }
}

// what every search is handed beside the prune launch's kept lists: the lengths, the shape, the trie and the outputs all share
struct BeamIo {
  const int32_t* lens;
  int64_t T;
  int C, blank, W, n_best;
  int2* trie;
  int32_t* tokens;
  int32_t* n_tokens;
  float* scores;
};

constexpr int kLmGroup = 4;                  // candidates per thread whose probes are in flight together

// ------------------------------------------------------------------ no scorer -------------------------------------------
// core.score is logaddexp(b, nb) itself: the acoustic score of a prefix and what it is ranked by are one array
struct NoCarry {};

struct NullScorer {
  struct Args {};
  struct Lds {
    BeamCore core;
  };
  using Carry = NoCarry;
  static constexpr Carry kNoCarry{};
  static constexpr bool kScored = false, kCutoff = false, kRerank = false;
  static constexpr int kOuts = 1;
  static constexpr const char* kName = "beam_search_kernel";
  struct Group {};
  static bool args_set(const Args&) { return true; }
  static __device__ __forceinline__ float* ascore(Lds& s) { return s.core.score; }
  __device__ __forceinline__ float* extra_out(int) const { return nullptr; }
  __device__ __forceinline__ bool open(const BeamIo&, const Args&) { return true; }
  __device__ __forceinline__ void init_root(Lds&) const {}
  __device__ __forceinline__ void begin_frame(Lds&, const BeamFetch&, int) const {}
  __device__ __forceinline__ void clear(Group&, int) const {}
  __device__ __forceinline__ void issue(const Lds&, Group&, int, int, int, int, int, float) const {}
  __device__ __forceinline__ void chain(const Lds&, Group&, int, const int (&)[kLmGroup]) const {}
  __device__ __forceinline__ float finish(const Lds&, Group&, int, int, int, int, int, float am, Carry*) const { return am; }
  static __device__ __forceinline__ void on_keep(Lds&, uint32_t, Carry) {}
  __device__ __forceinline__ void keep_entry(Lds&, int, int, int, int) const {}
  __device__ __forceinline__ void new_entry(Lds&, int, int, int, int, int, int, int) const {}
  __device__ __forceinline__ void final_scores(const Lds& s, int cur, int tid, float (&out)[kOuts]) const {
    out[0] = lae(s.core.b[cur][tid], s.core.nb[cur][tid]);
  }
};

// ------------------------------------------------------------------ n-gram LM images ------------------------------------
// A character LM scores an extension p -> p+c by lm(c | ctx(p)) = log10 p(longest stored (x_m .. x_1 c)) + sum of the backoffs
// of the longer stored contexts, found by a walk leftward from c through the image's hash, one probe per word.  An entry keeps
// the LM word ids of its last N-1 labels (words, for the word LM) and the backoff sums of its context chain.
constexpr int kLmMaxCtx = host::kArpaMaxOrder - 1;
constexpr float kLmOov = -1000.f;            // ctc_decoders' OOV_SCORE (natural log, not converted)
constexpr float kLmLogE = 0.4342944819f;     // ctc_decoders' NUM_FLT_LOGE: log10 -> natural log by division

__device__ __forceinline__ uint64_t lm_hash(uint64_t k) {   // == host::arpa_hash
  k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
  k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

struct LmImg {
  const float2* uni;
  const int32_t* cls;
  const uint4* slot;          // ArpaSlot as (key lo, key hi, lp bits, bow bits)
  uint32_t mask, n_words, n_classes;
  int nctx, bos, eos;
  bool ok;
};

// magic: the kind of image the calling search reads (a character image, or a word image with its lexicon)
__device__ __forceinline__ LmImg lm_open(const void* image, uint32_t magic = host::kArpaImageMagic) {
  const host::ArpaImageHeader* h = static_cast<const host::ArpaImageHeader*>(image);
  const char* base = static_cast<const char*>(image);
  LmImg m;
  m.ok = h->magic == magic && h->order >= 1 && h->order <= (uint32_t)host::kArpaMaxOrder &&
         h->log2_slots >= 4 && h->log2_slots < 32;
  m.uni = reinterpret_cast<const float2*>(base + h->uni_off);
  m.cls = reinterpret_cast<const int32_t*>(base + h->cls_off);
  m.slot = reinterpret_cast<const uint4*>(base + h->slot_off);
  m.mask = m.ok ? (1u << h->log2_slots) - 1u : 0u;
  m.n_words = h->n_words;
  m.n_classes = h->n_classes;
  m.nctx = m.ok ? (int)h->order - 1 : 0;
  m.bos = h->bos < h->n_words ? (int)h->bos : -1;
  m.eos = h->eos < h->n_words ? (int)h->eos : -1;
  return m;
}

// one probe for (suffix index g, word w): slot index + n_words of the stored n-gram, or -1; v = its slot
__device__ __forceinline__ int64_t lm_probe_rest(const LmImg& m, uint64_t key, uint32_t at, uint4 v, uint4* out) {
  while (true) {
    const uint64_t k = (uint64_t)v.x | ((uint64_t)v.y << 32);
    if (k == key) { *out = v; return (int64_t)m.n_words + at; }
    if (k == host::kArpaEmptyKey) return -1;
    at = (at + 1) & m.mask;
    v = m.slot[at];
  }
}

__device__ __forceinline__ int64_t lm_probe(const LmImg& m, int64_t g, int w, uint4* out) {
  const uint64_t key = ((uint64_t)g << 32) | (uint32_t)w;
  const uint32_t at = (uint32_t)lm_hash(key) & m.mask;
  return lm_probe_rest(m, key, at, m.slot[at], out);
}

// natural-log lm(w | ctx) from an entry's context ids (nearest first) and backoff sums; the single-chain form
__device__ float lm_score_one(const LmImg& m, int w, const int* ctx, const float* cb) {
  if (w < 0) return kLmOov;
  for (int d = 0; d < m.nctx; ++d)
    if (ctx[d] < 0) return kLmOov;
  int64_t g = w;
  float lp = m.uni[w].x;
  int mm = 0;
  for (int d = 0; d < m.nctx; ++d) {
    uint4 v;
    const int64_t f = lm_probe(m, g, ctx[d], &v);
    if (f < 0) break;
    g = f;
    lp = __uint_as_float(v.z);
    mm = d + 1;
  }
  return (lp + cb[mm]) / kLmLogE;
}

// the backoff sums of the context (w, ctx[0], .., ctx[nctx-2]) - the context of an entry whose last label is w
__device__ void lm_context_sums(const LmImg& m, int w, const int* ctx, float* cb) {
  float bows[kLmMaxCtx + 1];
  for (int j = 0; j <= kLmMaxCtx; ++j) bows[j] = 0.f;
  if (w >= 0 && m.nctx > 0) {
    bows[1] = m.uni[w].y;
    int64_t g = w;
    for (int d = 1; d < m.nctx; ++d) {
      if (ctx[d - 1] < 0) break;
      uint4 v;
      const int64_t f = lm_probe(m, g, ctx[d - 1], &v);
      if (f < 0) break;
      g = f;
      bows[d + 1] = __uint_as_float(v.w);
    }
  }
  float acc = 0.f;
  cb[m.nctx] = 0.f;
  for (int j = m.nctx - 1; j >= 0; --j) {
    acc += bows[j + 1];
    cb[j] = acc;
  }
}

// An entry's context chain in LDS, for both LM scorers: S has ctx[2][kLmMaxCtx][] (LM ids of the last N-1 labels or words,
// nearest first, -1 = OOV) and cb[2][kLmMaxCtx + 1][] (cb[j]: log10 backoffs of the stored contexts longer than j words).
template <class S>
__device__ __forceinline__ void lm_chain_load(const S& s, int cur, int i, int* cx, float* cb) {
  for (int d = 0; d < kLmMaxCtx; ++d) cx[d] = s.ctx[cur][d][i];
  for (int d = 0; d <= kLmMaxCtx; ++d) cb[d] = s.cb[cur][d][i];
}
template <class S>
__device__ __forceinline__ void lm_chain_copy(S& s, int cur, int nxt, int rank, int i) {
  for (int d = 0; d < kLmMaxCtx; ++d) s.ctx[nxt][d][rank] = s.ctx[cur][d][i];
  for (int d = 0; d <= kLmMaxCtx; ++d) s.cb[nxt][d][rank] = s.cb[cur][d][i];
}
// cb holds nctx + 1 sums; the rest of an entry's is 0
template <class S>
__device__ __forceinline__ void lm_chain_store(S& s, int nxt, int rank, const int* cx, const float* cb, int nctx) {
  for (int d = 0; d < kLmMaxCtx; ++d) s.ctx[nxt][d][rank] = cx[d];
  for (int d = 0; d <= kLmMaxCtx; ++d) s.cb[nxt][d][rank] = d <= nctx ? cb[d] : 0.f;
}
// the root's chain: <s> in every position
template <class S>
__device__ __forceinline__ void lm_chain_root(S& s, const LmImg& lm, bool ok) {
  int rc[kLmMaxCtx];
  float cb[kLmMaxCtx + 1];
  for (int d = 0; d < kLmMaxCtx; ++d) rc[d] = lm.bos;
  for (int d = 0; d <= kLmMaxCtx; ++d) cb[d] = 0.f;
  if (ok) lm_context_sums(lm, lm.bos, rc, cb);
  lm_chain_store(s, 0, 0, rc, cb, lm.nctx);
}
// the chain of p + w: w joins p's context
template <class S>
__device__ __forceinline__ void lm_chain_push(const S& s, const LmImg& lm, int cur, int p, int w, int* nc, float* cb) {
  nc[0] = w;
  for (int d = 1; d < kLmMaxCtx; ++d) nc[d] = s.ctx[cur][d - 1][p];
  lm_context_sums(lm, w, nc + 1, cb);
}
// ctc_decoders' sentence-end window of entry tid: </s> (and the <s> window of <s>^N </s> for an empty hypothesis)
template <class S>
__device__ __forceinline__ float lm_sentence_end(const S& s, const LmImg& lm, int cur, int tid) {
  int cx[kLmMaxCtx];
  float cb[kLmMaxCtx + 1];
  lm_chain_load(s, cur, tid, cx, cb);
  float sent = lm_score_one(lm, lm.eos, cx, cb);
  if (s.core.len[cur][tid] == 0) sent += lm_score_one(lm, lm.bos, cx, cb);
  return sent;
}

// the kernel arguments of the LM scorers (bias_image / bias_scores: LmScorer<true> alone)
struct LmArgs {
  const float* logp;
  const void* image;
  float alpha, beta;
  float* am_scores;
  const void* bias_image;
  float* bias_scores;
};

// ------------------------------------------------------------------ hotword biasing ------------------------------------
// hotword_io.h has the automaton, its image and the walker.  Each entry carries the automaton node of its prefix and
// bonus(prefix); like the LM bonus both depend on the prefix alone, so merging stays exact.  step(root, c) of every kept label is
// resolved once per frame into LDS: most live entries sit at the root and then cost no global probe per candidate.  The first
// probes of a thread's other candidates are loaded together, kLmGroup at a time, and handed to the walker.  A survivor's step is
// walked again when its entry is written, so no candidate carries its next node in registers.  A bank of no phrases (one node)
// switches every probe off.
struct BiasImg {
  host::HotwordView m;
  bool ok, on;                // ok: a hotword image for these classes; on: it holds a phrase
};

__device__ __forceinline__ BiasImg bias_open(const void* image, int C, int blank) {
  BiasImg b;
  b.m = host::hotword_open(image, 0);
  b.ok = b.m.ok && b.m.n_classes == (uint32_t)C && b.m.blank == (uint32_t)blank;
  b.on = b.ok && b.m.n_nodes > 1;
  return b;
}

struct BiasLds {
  int state[2][kBeamMaxWidth];                           // automaton node of each entry's prefix (0: the root)
  float bonus[2][kBeamMaxWidth];                         // bonus(prefix): the sum of its steps' deltas
  int rchild[kBeamMaxTopN], rstate[kBeamMaxTopN];        // per kept label: the root's child by it (-1: none) and step(root, label)
  float rdelta[kBeamMaxTopN];
  float fin[3][kBeamMaxWidth];                           // the re-ranked final score, am_scores and bias_scores values
};

// step(root, c) of the kept label this thread fetched (tid < n): c = BeamFetch::pc before beam_fetch_frame publishes it
__device__ __forceinline__ void bias_root_steps(const BiasImg& hw, BiasLds& s, int tid, int n, int c, int blank) {
  if (tid >= n) return;
  int child = -1, st = 0;
  float d = 0.f;
  if (hw.on && c != blank && c >= 0 && (uint32_t)c < hw.m.n_classes) {
    child = host::hotword_child(hw.m, 0, c);
    st = host::hotword_step(hw.m, 0, c, child, host::HotwordEdge{}, &d);
  }
  s.rchild[tid] = child; s.rstate[tid] = st; s.rdelta[tid] = d;
}

// the slot the walk of (entry p, label c) probes first: loaded ahead of bias_walk, for several candidates at once.  Held as
// (key, child) so that a thread's group of them stays in registers.
struct BiasFirst {
  uint64_t key;
  int32_t child;
};

__device__ __forceinline__ BiasFirst bias_first(const BiasImg& hw, const BiasLds& s, int cur, int p, int c) {
  const int v = s.state[cur][p];
  if (!hw.on || v == 0) return BiasFirst{host::kHotwordEmptyKey, -1};
  const uint4 e = *reinterpret_cast<const uint4*>(&hw.m.edge[host::hotword_slot(hw.m, v, c)]);
  return BiasFirst{(uint64_t)e.x | ((uint64_t)e.y << 32), (int32_t)e.z};
}

// step(state(p), kept[k] = c): the node p+c reaches; *delta = bonus(p+c) - bonus(p)
__device__ __forceinline__ int bias_walk(const BiasImg& hw, const BiasLds& s, int cur, int p, int k, int c,
                                         uint64_t first_key, int32_t first_child, float* delta) {
  const int v = s.state[cur][p];
  if (!hw.on) { *delta = 0.f; return 0; }
  if (v == 0) { *delta = s.rdelta[k]; return s.rstate[k]; }
  host::HotwordEdge first;
  first.key = first_key; first.child = first_child; first.reserved = 0;
  return host::hotword_step(hw.m, v, c, s.rchild[k], first, delta);
}

// The hotword share of a search: BiasScorer is this alone, LmScorer<true> has it beside the character LM.
struct BiasPart {
  BiasImg hw;
  struct Group {
    uint64_t key[kLmGroup];
    int32_t child[kLmGroup];
  };
  __device__ __forceinline__ void init_root(BiasLds& s) const { s.state[0][0] = 0; s.bonus[0][0] = 0.f; }
  __device__ __forceinline__ void clear(Group& g, int u) const { g.key[u] = host::kHotwordEmptyKey; g.child[u] = -1; }
  __device__ __forceinline__ void issue(const BiasLds& s, Group& g, int u, int cur, int p, int c) const {
    const BiasFirst e = bias_first(hw, s, cur, p, c);
    g.key[u] = e.key; g.child[u] = e.child;
  }
  // bonus(p + c) - bonus(p) of the candidate whose first probe issue() loaded
  __device__ __forceinline__ float delta(const BiasLds& s, const Group& g, int u, int cur, int p, int k, int c) const {
    float hd;
    bias_walk(hw, s, cur, p, k, c, g.key[u], g.child[u], &hd);
    return hd;
  }
  __device__ __forceinline__ void keep_entry(BiasLds& s, int cur, int nxt, int rank, int i) const {
    s.state[nxt][rank] = s.state[cur][i]; s.bonus[nxt][rank] = s.bonus[cur][i];
  }
  __device__ __forceinline__ void new_entry(BiasLds& s, int cur, int nxt, int rank, int p, int k, int c) const {
    float hd;
    const BiasFirst e = bias_first(hw, s, cur, p, c);
    s.state[nxt][rank] = bias_walk(hw, s, cur, p, k, c, e.key, e.child, &hd);
    s.bonus[nxt][rank] = s.bonus[cur][p] + hd;
  }
  // end of utterance: an unfinished match gives its provisional credit back
  __device__ __forceinline__ float final_bonus(const BiasLds& s, int cur, int tid) const {
    return s.bonus[cur][tid] + (hw.on ? host::hotword_give_back(hw.m, s.state[cur][tid]) : 0.f);
  }
};

// lasr_ctc_beam_decode_bias: core.score is logaddexp(b, nb) + bonus(prefix).  With a bank of no phrases every bonus is 0 and
// each score is the expression NullScorer's search evaluates, so the result is that search's bit for bit.
struct BiasScorer {
  struct Args {
    const void* bias_image;
    float* am_scores;
    float* bias_scores;
  };
  struct Lds {
    BeamCore core;
    float ascore[kBeamMaxWidth];                           // acoustic logaddexp(b, nb) of the current beam
    BiasLds hw;
  };
  using Carry = NoCarry;
  static constexpr Carry kNoCarry{};
  static constexpr bool kScored = true, kCutoff = false, kRerank = true;
  static constexpr int kOuts = 3;
  static constexpr const char* kName = "beam_search_bias_kernel";
  using Group = BiasPart::Group;
  BiasPart bias;
  Args a;
  int blank;
  static bool args_set(const Args& a) { return a.bias_image && a.am_scores && a.bias_scores; }
  static __device__ __forceinline__ float* ascore(Lds& s) { return s.ascore; }
  static __device__ __forceinline__ auto& fin(Lds& s) { return s.hw.fin; }
  __device__ __forceinline__ float* extra_out(int n) const { return n == 1 ? a.am_scores : a.bias_scores; }
  __device__ __forceinline__ bool open(const BeamIo& io, const Args& args) {
    a = args; blank = io.blank;
    bias.hw = bias_open(a.bias_image, io.C, io.blank);
    return bias.hw.ok;
  }
  __device__ __forceinline__ void init_root(Lds& s) const { bias.init_root(s.hw); }
  __device__ __forceinline__ void begin_frame(Lds& s, const BeamFetch& pf, int tid) const {
    bias_root_steps(bias.hw, s.hw, tid, pf.pn, pf.pc, blank);
  }
  __device__ __forceinline__ float prefix_bonus(const Lds& s, int cur, int i) const { return s.hw.bonus[cur][i]; }
  __device__ __forceinline__ void prefix_extras(Lds&, int, int) const {}
  __device__ __forceinline__ void clear(Group& g, int u) const { bias.clear(g, u); }
  __device__ __forceinline__ void issue(const Lds& s, Group& g, int u, int cur, int p, int, int c, float) const {
    bias.issue(s.hw, g, u, cur, p, c);
  }
  __device__ __forceinline__ void chain(const Lds&, Group&, int, const int (&)[kLmGroup]) const {}
  __device__ __forceinline__ float finish(const Lds& s, Group& g, int u, int cur, int p, int k, int c, float am, Carry*) const {
    return am + (s.hw.bonus[cur][p] + bias.delta(s.hw, g, u, cur, p, k, c));
  }
  static __device__ __forceinline__ void on_keep(Lds&, uint32_t, Carry) {}
  __device__ __forceinline__ void keep_entry(Lds& s, int cur, int nxt, int rank, int i) const {
    bias.keep_entry(s.hw, cur, nxt, rank, i);
  }
  __device__ __forceinline__ void new_entry(Lds& s, int cur, int nxt, int rank, int p, int k, int c, int) const {
    bias.new_entry(s.hw, cur, nxt, rank, p, k, c);
  }
  __device__ __forceinline__ void final_scores(const Lds& s, int cur, int tid, float (&out)[kOuts]) const {
    const float am = lae(s.core.b[cur][tid], s.core.nb[cur][tid]);
    const float fb = bias.final_bonus(s.hw, cur, tid);
    out[0] = am + fb; out[1] = am; out[2] = fb;
  }
};

// ------------------------------------------------------------------ character n-gram LM (+ hotwords) -------------------
// lasr_ctc_beam_decode_lm / _lm_bias: ctc_decoders' character-based Scorer.  Beside the acoustic log_b / log_nb an entry keeps
// its LM bonus (alpha * sum of lm + beta * labels, which depends on the prefix alone, so merging stays exact), its own emission
// term and its context chain; the probes of a thread's kLmGroup candidates go out together.  kBias: the hotword share
// (BiasPart) beside it; every statement of the biasing is under `if constexpr (kBias)`.
struct BeamLmLds {
  BeamCore core;
  float surv_t[kBeamMaxWidth];                           // emission term of a surviving extension (beside core.surv_i)
  float bonus[2][kBeamMaxWidth], term[2][kBeamMaxWidth]; // alpha * sum lm + beta * labels; the last label's own term
  int ctx[2][kLmMaxCtx][kBeamMaxWidth];
  float cb[2][kLmMaxCtx + 1][kBeamMaxWidth];
  float ascore[kBeamMaxWidth];                           // acoustic logaddexp(b, nb) of the current beam
  int kwid[kBeamMaxTopN];                                // LM word id of each kept label (-1: the blank, or not in the LM)
  int ctx_oov[kBeamMaxWidth];
};
struct BeamLmBiasLds : BeamLmLds {
  BiasLds hw;
};

template <bool kBias>
struct LmScorer {
  using Args = LmArgs;
  using Lds = std::conditional_t<kBias, BeamLmBiasLds, BeamLmLds>;
  using Carry = float;                                   // the extension's emission term
  static constexpr Carry kNoCarry = 0.f;
  static constexpr bool kScored = true, kCutoff = true, kRerank = kBias;
  static constexpr int kOuts = kBias ? 3 : 2;
  static constexpr const char* kName = kBias ? "beam_search_lm_kernel (biased)" : "beam_search_lm_kernel";
  struct Group {
    float lpv[kLmGroup];
    int64_t g[kLmGroup];
    int mm[kLmGroup], wc[kLmGroup];
    bool act[kLmGroup];
    std::conditional_t<kBias, BiasPart::Group, NoCarry> hw;
  };
  LmImg lm;
  BiasPart bias;
  Args a;
  const float* logp;
  int blank;
  static bool args_set(const Args& a) { return a.image && a.am_scores && (!kBias || (a.bias_image && a.bias_scores)); }
  static __device__ __forceinline__ float* ascore(Lds& s) { return s.ascore; }
  static __device__ __forceinline__ auto& fin(Lds& s) { return s.hw.fin; }
  __device__ __forceinline__ float* extra_out(int n) const { return n == 1 ? a.am_scores : a.bias_scores; }
  __device__ __forceinline__ bool open(const BeamIo& io, const Args& args) {
    a = args; logp = args.logp; blank = io.blank;
    lm = lm_open(a.image);
    if constexpr (kBias) {
      bias.hw = bias_open(a.bias_image, io.C, io.blank);
      lm.ok = lm.ok && bias.hw.ok;          // either image wrong: empty slots
    }
    return lm.ok;
  }
  // the early cutoff's slack: one label's beta, and with hotwords one step of the automaton
  __device__ __forceinline__ float cut_slack() const {
    float slack = fmaxf(0.f, a.beta);
    if constexpr (kBias) slack += bias.hw.m.max_credit;
    return slack;
  }
  __device__ __forceinline__ void init_root(Lds& s) const {
    s.bonus[0][0] = 0.f; s.term[0][0] = 0.f;
    if constexpr (kBias) bias.init_root(s.hw);
    lm_chain_root(s, lm, lm.ok);
  }
  __device__ __forceinline__ void begin_frame(Lds& s, const BeamFetch& pf, int tid) const {
    if (tid < pf.pn) s.kwid[tid] = (pf.pc != blank && pf.pc >= 0 && (uint32_t)pf.pc < lm.n_classes) ? lm.cls[pf.pc] : -1;
    if constexpr (kBias) bias_root_steps(bias.hw, s.hw, tid, pf.pn, pf.pc, blank);
  }
  __device__ __forceinline__ float prefix_bonus(const Lds& s, int cur, int i) const {
    if constexpr (kBias) return s.bonus[cur][i] + s.hw.bonus[cur][i];
    else return s.bonus[cur][i];
  }
  __device__ __forceinline__ void prefix_extras(Lds& s, int cur, int tid) const {
    int oov = 0;
    for (int d = 0; d < lm.nctx; ++d) oov |= s.ctx[cur][d][tid] < 0;
    s.ctx_oov[tid] = oov;
  }
  __device__ __forceinline__ void clear(Group& g, int u) const {
    g.lpv[u] = 0.f; g.g[u] = 0; g.mm[u] = 0; g.wc[u] = -1; g.act[u] = false;
    if constexpr (kBias) bias.clear(g.hw, u);
  }
  __device__ __forceinline__ void issue(const Lds& s, Group& g, int u, int cur, int p, int k, int c, float) const {
    g.wc[u] = s.kwid[k];
    if constexpr (kBias) bias.issue(s.hw, g.hw, u, cur, p, c);
    if (g.wc[u] >= 0 && !s.ctx_oov[p]) {
      g.g[u] = g.wc[u];
      g.lpv[u] = lm.uni[g.wc[u]].x;
      g.act[u] = lm.nctx > 0;
    }
  }
  // the group's walks leftward, one context word per round: every probe of a round is loaded before any is compared
  __device__ __forceinline__ void chain(const Lds& s, Group& g, int cur, const int (&pp)[kLmGroup]) const {
    for (int d = 0; d < lm.nctx; ++d) {
      uint64_t key[kLmGroup];
      uint32_t at[kLmGroup];
      uint4 v[kLmGroup];
#pragma unroll
      for (int u = 0; u < kLmGroup; ++u) {
        if (!g.act[u]) continue;
        key[u] = ((uint64_t)g.g[u] << 32) | (uint32_t)s.ctx[cur][d][pp[u]];
        at[u] = (uint32_t)lm_hash(key[u]) & lm.mask;
        v[u] = lm.slot[at[u]];
      }
#pragma unroll
      for (int u = 0; u < kLmGroup; ++u) {
        if (!g.act[u]) continue;
        uint4 hit;
        const int64_t f = lm_probe_rest(lm, key[u], at[u], v[u], &hit);
        if (f < 0) {
          g.act[u] = false;
        } else {
          g.g[u] = f;
          g.lpv[u] = __uint_as_float(hit.z);
          g.mm[u] = d + 1;
        }
      }
    }
  }
  __device__ __forceinline__ float finish(const Lds& s, Group& g, int u, int cur, int p, int k, int c, float am, Carry* term) const {
    const bool oov = g.wc[u] < 0 || s.ctx_oov[p];
    const float lmv = oov ? kLmOov : (g.lpv[u] + s.cb[cur][g.mm[u]][p]) / kLmLogE;
    *term = a.alpha * lmv + a.beta;
    if constexpr (kBias) return am + ((s.bonus[cur][p] + *term) + (s.hw.bonus[cur][p] + bias.delta(s.hw, g.hw, u, cur, p, k, c)));
    else return am + (s.bonus[cur][p] + *term);
  }
  static __device__ __forceinline__ void on_keep(Lds& s, uint32_t pos, Carry term) { s.surv_t[pos] = term; }
  __device__ __forceinline__ void keep_entry(Lds& s, int cur, int nxt, int rank, int i) const {
    s.bonus[nxt][rank] = s.bonus[cur][i]; s.term[nxt][rank] = s.term[cur][i];
    if constexpr (kBias) bias.keep_entry(s.hw, cur, nxt, rank, i);
    lm_chain_copy(s, cur, nxt, rank, i);
  }
  __device__ __forceinline__ void new_entry(Lds& s, int cur, int nxt, int rank, int p, int k, int c, int tid) const {
    const float tm = s.surv_t[tid];
    s.bonus[nxt][rank] = s.bonus[cur][p] + tm; s.term[nxt][rank] = tm;
    if constexpr (kBias) bias.new_entry(s.hw, cur, nxt, rank, p, k, c);
    int nc[kLmMaxCtx];
    float cb[kLmMaxCtx + 1];
    lm_chain_push(s, lm, cur, p, s.kwid[k], nc, cb);
    lm_chain_store(s, nxt, rank, nc, cb, lm.nctx);
  }
  // ctc_decoders' approx_ctc = fused - k beta - alpha sent_lm: the emission terms cancel, the sentence-end window remains
  __device__ __forceinline__ void final_scores(const Lds& s, int cur, int tid, float (&out)[kOuts]) const {
    const float as = lae(s.core.b[cur][tid], s.core.nb[cur][tid]);
    const float sent = lm_sentence_end(s, lm, cur, tid);
    if constexpr (kBias) {
      const float fb = bias.final_bonus(s.hw, cur, tid);
      out[0] = as + (s.bonus[cur][tid] + fb);
      out[2] = fb;
    } else {
      out[0] = as + s.bonus[cur][tid];
    }
    out[1] = as - a.alpha * sent;
  }
};

// ------------------------------------------------------------------ word n-gram LM and its lexicon ---------------------
// lasr_ctc_beam_decode_wlm: each entry carries the lexicon trie node of its unfinished word; p + c exists only where that node
// has a child c, p + space only where it is a complete word, and the LM scores a word when the space after it is emitted.  What
// a prefix needs in every frame is worked out once, when its entry is created: its node, the LM id of the word the node spells
// and `sterm`, the term the space after that word adds (alpha * lm(word | context) + beta) - also the end-of-utterance term.  A
// frame then costs one lexicon probe per (prefix, kept label) candidate, kLmGroup of them in flight per thread, and one n-gram
// chain per NEW prefix.
struct WlmImg {
  LmImg lm;
  const uint4* edge;          // ArpaLexEdge as (key lo, key hi, child, reserved)
  const int32_t* node_word;
  uint32_t emask;
  int space;
};

__device__ __forceinline__ WlmImg wlm_open(const void* image) {
  WlmImg w;
  w.lm = lm_open(image, host::kArpaWordImageMagic);
  const host::ArpaLexHeader* h =
      reinterpret_cast<const host::ArpaLexHeader*>(static_cast<const char*>(image) + sizeof(host::ArpaImageHeader));
  const char* base = static_cast<const char*>(image);
  w.lm.ok = w.lm.ok && h->log2_edges >= 4 && h->log2_edges < 32 && h->n_nodes >= 1;
  w.edge = reinterpret_cast<const uint4*>(base + (w.lm.ok ? h->edge_off : 0));
  w.node_word = reinterpret_cast<const int32_t*>(base + (w.lm.ok ? h->node_off : 0));
  w.emask = w.lm.ok ? (1u << h->log2_edges) - 1u : 0u;
  w.space = w.lm.ok ? (int)h->space_id : -1;
  return w;
}

// the child of `key` = node << 32 | class, or -1; v = the edge slot at `at`, already loaded
__device__ __forceinline__ int wlm_child_rest(const WlmImg& w, uint64_t key, uint32_t at, uint4 v) {
  while (true) {
    const uint64_t k = (uint64_t)v.x | ((uint64_t)v.y << 32);
    if (k == key) return (int)v.z;
    if (k == host::kArpaEmptyKey) return -1;
    at = (at + 1) & w.emask;
    v = w.edge[at];
  }
}

struct WlmScorer {
  using Args = LmArgs;
  struct Lds {
    BeamCore core;
    int surv_n[kBeamMaxWidth];                             // lexicon node of a surviving extension (beside core.surv_i)
    int lex[2][kBeamMaxWidth], wid[2][kBeamMaxWidth];      // trie node of the unfinished word; the LM word it spells, or -1
    float bonus[2][kBeamMaxWidth], sterm[2][kBeamMaxWidth];// sum of the terms of the prefix's spaces; the next space's term
    int ctx[2][kLmMaxCtx][kBeamMaxWidth];                  // the last N-1 finished words
    float cb[2][kLmMaxCtx + 1][kBeamMaxWidth];
    float ascore[kBeamMaxWidth];                           // acoustic logaddexp(b, nb) of the current beam
    float fin[2][kBeamMaxWidth];                           // the re-ranked final score (end term included) and am_scores values
  };
  using Carry = int;                                       // the lexicon node the extension reaches
  static constexpr Carry kNoCarry = -1;
  static constexpr bool kScored = true, kCutoff = true, kRerank = true;
  static constexpr int kOuts = 2;
  static constexpr const char* kName = "beam_search_wlm_kernel";
  struct Group {
    float sc[kLmGroup];
    uint64_t key[kLmGroup];
    uint32_t at[kLmGroup];
    uint4 v[kLmGroup];
    int child[kLmGroup];
    bool probe[kLmGroup];
  };
  WlmImg wl;
  Args a;
  const float* logp;
  static bool args_set(const Args& a) { return a.image && a.am_scores; }
  static __device__ __forceinline__ float* ascore(Lds& s) { return s.ascore; }
  static __device__ __forceinline__ auto& fin(Lds& s) { return s.fin; }
  __device__ __forceinline__ float* extra_out(int) const { return a.am_scores; }
  __device__ __forceinline__ bool open(const BeamIo& io, const Args& args) {
    a = args; logp = args.logp;
    wl = wlm_open(a.image);
    wl.lm.ok = wl.lm.ok && wl.space >= 0 && wl.space < io.C && wl.space != io.blank;
    return wl.lm.ok;
  }
  __device__ __forceinline__ float cut_slack() const { return fmaxf(0.f, a.beta); }
  __device__ __forceinline__ void init_root(Lds& s) const {
    s.bonus[0][0] = 0.f; s.sterm[0][0] = 0.f; s.lex[0][0] = 0; s.wid[0][0] = -1;
    lm_chain_root(s, wl.lm, wl.lm.ok);
  }
  __device__ __forceinline__ void begin_frame(Lds&, const BeamFetch&, int) const {}
  __device__ __forceinline__ float prefix_bonus(const Lds& s, int cur, int i) const { return s.bonus[cur][i]; }
  __device__ __forceinline__ void prefix_extras(Lds&, int, int) const {}
  __device__ __forceinline__ void clear(Group& g, int u) const { g.sc[u] = kNegInfB; g.child[u] = -1; g.probe[u] = false; }
  __device__ __forceinline__ void issue(const Lds& s, Group& g, int u, int cur, int p, int, int c, float am) const {
    if (c == wl.space) {
      if (s.wid[cur][p] >= 0) {              // the node is a complete word: the space scores it and returns to the root
        g.child[u] = 0;
        g.sc[u] = am + (s.bonus[cur][p] + s.sterm[cur][p]);
      }
    } else {
      g.sc[u] = am + s.bonus[cur][p];
      g.key[u] = ((uint64_t)(uint32_t)s.lex[cur][p] << 32) | (uint32_t)c;
      g.at[u] = (uint32_t)lm_hash(g.key[u]) & wl.emask;
      g.v[u] = wl.edge[g.at[u]];
      g.probe[u] = true;
    }
  }
  __device__ __forceinline__ void chain(const Lds&, Group&, int, const int (&)[kLmGroup]) const {}
  __device__ __forceinline__ float finish(const Lds&, Group& g, int u, int, int, int, int, float, Carry* child) const {
    if (g.probe[u]) {
      g.child[u] = wlm_child_rest(wl, g.key[u], g.at[u], g.v[u]);
      if (g.child[u] < 0) g.sc[u] = kNegInfB;      // no such word in the lexicon
    }
    *child = g.child[u];
    return g.sc[u];
  }
  static __device__ __forceinline__ void on_keep(Lds& s, uint32_t pos, Carry child) { s.surv_n[pos] = child; }
  __device__ __forceinline__ void keep_entry(Lds& s, int cur, int nxt, int rank, int i) const {
    s.lex[nxt][rank] = s.lex[cur][i]; s.wid[nxt][rank] = s.wid[cur][i];
    s.bonus[nxt][rank] = s.bonus[cur][i]; s.sterm[nxt][rank] = s.sterm[cur][i];
    lm_chain_copy(s, cur, nxt, rank, i);
  }
  __device__ __forceinline__ void new_entry(Lds& s, int cur, int nxt, int rank, int p, int, int c, int tid) const {
    int nc[kLmMaxCtx];
    float cb[kLmMaxCtx + 1];
    if (c == wl.space) {
      // the word of p's node is finished: it joins the context, the trie state returns to the root
      lm_chain_push(s, wl.lm, cur, p, s.wid[cur][p], nc, cb);
      s.lex[nxt][rank] = 0; s.wid[nxt][rank] = -1;
      s.bonus[nxt][rank] = s.bonus[cur][p] + s.sterm[cur][p]; s.sterm[nxt][rank] = 0.f;
    } else {
      const int node = s.surv_n[tid];
      const int w = wl.node_word[node];
      lm_chain_load(s, cur, p, nc, cb);
      s.lex[nxt][rank] = node; s.wid[nxt][rank] = w;
      s.bonus[nxt][rank] = s.bonus[cur][p];
      s.sterm[nxt][rank] = w >= 0 ? a.alpha * lm_score_one(wl.lm, w, nc, cb) + a.beta : 0.f;
    }
    lm_chain_store(s, nxt, rank, nc, cb, wl.lm.nctx);
  }
  // end of utterance: an unfinished last word is scored (OOV_SCORE where the node is no complete word)
  __device__ __forceinline__ void final_scores(const Lds& s, int cur, int tid, float (&out)[kOuts]) const {
    const float as = lae(s.core.b[cur][tid], s.core.nb[cur][tid]);
    float f = as + s.bonus[cur][tid];
    if (s.core.len[cur][tid] > 0 && s.core.last[cur][tid] != wl.space)
      f += s.wid[cur][tid] >= 0 ? s.sterm[cur][tid] : a.alpha * kLmOov + a.beta;
    out[0] = f; out[1] = as;
  }
};

static_assert(sizeof(BeamLmBiasLds) < 64 * 1024 && sizeof(WlmScorer::Lds) < 64 * 1024, "static LDS of the widest searches");

// ------------------------------------------------------------------ the search: one-shot or resumable ------------------
// What a search does with its state between two launches is a Mode policy beside the Scorer.  OneShot: nothing, the beam lives
// and dies in LDS.  Streamed (lasr_ctc_beam_stream_feed): between two frames the whole state of a search is the scorer's LDS
// record (values and indices, no pointers), the trie and the registers nbeam and cur; a launch searches the frames of one chunk,
// and the workgroup loads that state when it starts and stores it when the chunk's last frame is done.  Per stream the
// caller's buffer holds a StreamHeader, the LDS image and the trie of T_cap frames (stream_layout).
struct StreamHeader {
  int32_t t0;         // frames searched so far: the next frame's trie nodes are 1 + t0 * W ..
  int32_t nbeam, cur;
  int32_t dropped;    // frames fed beyond T_cap: counted, never searched
  int32_t live;       // 0: the empty prefix (after a reset); the image and nbeam / cur mean nothing
  int32_t pad[11];
};
static_assert(sizeof(StreamHeader) == 64, "the LDS image behind the header stays 16-byte aligned");

struct OneShot {
  static constexpr bool kStream = false;
  struct Args {};
};

struct Streamed {
  static constexpr bool kStream = true;
  struct Args {
    char* state;                  // stream b: state + b * stride
    size_t stride, trie_off;      // the image is at sizeof(StreamHeader), the trie at trie_off
    int64_t T_cap;
    int32_t* n_frames;
    int32_t* n_dropped;
  };
};

// the LDS record to or from its image, 16 bytes per thread and round (every Lds is a multiple of 8 bytes; the image's size is
// rounded up to 16, and so is the static LDS allocation's granule)
template <class Lds, bool kStore>
__device__ __forceinline__ void stream_copy_lds(Lds& s, char* image, int tid) {
  constexpr int kWords = (int)(sizeof(Lds) / sizeof(uint32_t));
  static_assert(sizeof(Lds) % sizeof(uint32_t) == 0, "the LDS record is copied word by word");
  uint32_t* lds = reinterpret_cast<uint32_t*>(&s);
  uint32_t* img = reinterpret_cast<uint32_t*>(image);
  for (int i = tid; i < kWords; i += kSearchThreads) {
    if constexpr (kStore) img[i] = lds[i];
    else lds[i] = img[i];
  }
}

// ------------------------------------------------------------------ the search: one frame loop -------------------------
// The kept lists come as kernel parameters of their own, const and __restrict__, not inside BeamIo: only so does the compiler
// know that a frame's trie stores leave them alone, and the next frame's count, which every thread reads, is prefetched by a
// scalar load.  As a vector load it is waited for on the spot, and the kept list's prefetch with it.
//
// Mode = Streamed: io.T, io.lens, the kept lists and the scorer's logp are the CHUNK's, frames are indexed locally into them;
// the trie, the tokens' pitch and the node numbers go by T_cap and the stream's frame count.  Everything a frame computes reads
// the LDS record, nbeam, cur and that frame's kept list alone, so a sequence cut into chunks anywhere gives the frames the same
// inputs in the same order as one launch over the whole of it: the same tokens and the same f32 scores, bit for bit.
template <int J, class Scorer, class Mode = OneShot>
__global__ __launch_bounds__(kSearchThreads) void beam_search_kernel(const int32_t* __restrict__ kcls_g,
                                                                     const float* __restrict__ klp_g,
                                                                     const int32_t* __restrict__ kn_g, const BeamIo io,
                                                                     const typename Scorer::Args sargs,
                                                                     const typename Mode::Args margs) {
  __shared__ typename Scorer::Lds s;
  BeamCore& core = s.core;
  float* const asc = Scorer::ascore(s);     // acoustic logaddexp(b, nb) of the current beam: core.score itself without a scorer
  const int tid = threadIdx.x;
  const int64_t ub = blockIdx.x;
  const int64_t T = io.T;
  const int blank = io.blank, W = io.W, n_best = io.n_best;
  Scorer sc;
  const bool ok = sc.open(io, sargs);       // a wrong image: no frames, empty slots
  int64_t L = !ok ? 0 : io.lens ? min((int64_t)max(io.lens[ub], 0), T) : T;
  int64_t Tout = T;                         // the tokens' pitch and the trie's frames
  int2* trie;
  [[maybe_unused]] StreamHeader* hdr = nullptr;
  [[maybe_unused]] int t0 = 0, dropped = 0;
  [[maybe_unused]] bool live = false;
  if constexpr (Mode::kStream) {
    char* mine = margs.state + (size_t)ub * margs.stride;
    hdr = reinterpret_cast<StreamHeader*>(mine);
    trie = reinterpret_cast<int2*>(mine + margs.trie_off);
    Tout = margs.T_cap;
    live = hdr->live != 0;
    if (live) { t0 = min(max(hdr->t0, 0), (int)Tout); dropped = hdr->dropped; }
    const int64_t room = Tout - t0;         // the device's clamp: frames past T_cap are counted, not searched
    if (ok && L > room) { dropped += (int)(L - room); L = room; }
  } else {
    trie = io.trie + ub * (1 + T * (int64_t)W);
  }
  BeamFetch pf{kcls_g + ub * T * kBeamMaxTopN, klp_g + ub * T * kBeamMaxTopN, kn_g + ub * T};
  int nbeam = 1, cur = 0;
  bool resumed = false;
  if constexpr (Mode::kStream) {
    if (ok && live) {
      // the record as the last chunk's last frame left it (its histogram zeroed, as beam_init_root leaves it); the barrier
      // keeps begin_frame's and beam_fetch_frame's stores of this chunk's first frame behind the load
      stream_copy_lds<typename Scorer::Lds, false>(s, reinterpret_cast<char*>(hdr) + sizeof(StreamHeader), tid);
      nbeam = min(max(hdr->nbeam, 0), W);
      cur = hdr->cur & 1;
      resumed = true;
      __syncthreads();
    }
  }
  if (!resumed) {
    beam_init_root(core, tid);
    if (tid == 0) sc.init_root(s);
  }
  // the early cutoff's reference, the frame's unpruned blank log-prob, is fetched a frame ahead like the kept list
  [[maybe_unused]] const float* lrow = nullptr;
  [[maybe_unused]] float pblank = 0.f, cut_slack = 0.f;
  if constexpr (Scorer::kCutoff) {
    lrow = sc.logp + ub * T * (int64_t)io.C;
    cut_slack = sc.cut_slack();
  }
  if (L > 0) {
    pf.request(0, tid);
    if constexpr (Scorer::kCutoff) pblank = lrow[blank];
  }
  for (int64_t t = 0; t < L; ++t) {
    [[maybe_unused]] const float lblank = pblank;
    sc.begin_frame(s, pf, tid);
    const int nk = beam_fetch_frame(core, pf, t, L, tid);
    if constexpr (Scorer::kCutoff) {
      if (t + 1 < L) pblank = lrow[(t + 1) * (int64_t)io.C + blank];
    }
    __syncthreads();
    // (1) per live prefix: scores, kept index of its last label and of the blank, its parent among the live entries
    int lastk = -1, pr = -1;
    float blp = kNegInfB;
    if (tid < nbeam) {
      const int last = core.last[cur][tid];
      const float as = lae(core.b[cur][tid], core.nb[cur][tid]);
      asc[tid] = as;
      if constexpr (Scorer::kScored) {
        core.score[tid] = as + sc.prefix_bonus(s, cur, tid);
        sc.prefix_extras(s, cur, tid);
      }
      beam_lookup(core, cur, nbeam, nk, blank, tid, last, &lastk, &pr, &blp);
    }
    __syncthreads();
    // the early cutoff: with a full beam, (p, c) contributes nothing where score(p) + logp[c] < min_cutoff
    [[maybe_unused]] float min_cutoff = kNegInfB;
    if constexpr (Scorer::kCutoff) min_cutoff = nbeam == W ? core.score[W - 1] + lblank - cut_slack : kNegInfB;
    auto cut = [&](int p, float lc) {
      if constexpr (Scorer::kCutoff) return core.score[p] + lc < min_cutoff;
      else return false;
    };
    // (2) "no new label" candidates (acoustic), with the parent's extension by the last label folded in
    if (tid < nbeam) {
      const float as = asc[tid];
      float nbn = kNegInfB;
      if (lastk >= 0) {
        const float lc = core.klp[lastk];
        if (!cut(tid, lc)) nbn = lc + core.nb[cur][tid];
        if (pr >= 0) {
          if (!cut(pr, lc)) nbn = lae(nbn, lc + (core.last[cur][tid] == core.last[cur][pr] ? core.b[cur][pr] : asc[pr]));
          atomicOr(&core.merged[pr], 1ull << lastk);
        }
      }
      core.next_b[tid] = blp + as;
      core.next_nb[tid] = nbn;
    }
    __syncthreads();
    // (3) candidates: i < nbeam "no new label" of entry i, then nbeam * nk extensions (p, k); composite = score desc, key
    // asc.  The scorer's probes of kLmGroup extensions per thread are issued together, then consumed.
    const int ncand = nbeam + nbeam * nk;
    uint64_t comp[J];
    typename Scorer::Carry carry[J];
    uint64_t valid = 0;
#pragma unroll
    for (int j0 = 0; j0 < J; j0 += kLmGroup) {
      typename Scorer::Group g;
      float am[kLmGroup];
      uint32_t ck[kLmGroup];
      int pp[kLmGroup], kk[kLmGroup];
      bool ext[kLmGroup];
#pragma unroll
      for (int u = 0; u < kLmGroup; ++u) {
        const int j = j0 + u;
        am[u] = kNegInfB; ck[u] = 0; pp[u] = 0; kk[u] = 0; ext[u] = false;
        sc.clear(g, u);
        if (j >= J) continue;
        const int i = tid + j * kSearchThreads;
        if (i < nbeam) {
          am[u] = lae(core.next_b[i], core.next_nb[i]);
          if constexpr (Scorer::kScored) am[u] = am[u] + sc.prefix_bonus(s, cur, i);
          ck[u] = (uint32_t)i << 14;
        } else if (i < ncand) {
          const int q = i - nbeam, p = q / nk, k = q - p * nk;
          const int c = core.kcls[k];
          pp[u] = p; kk[u] = k;
          ck[u] = ((uint32_t)p << 14) | (uint32_t)(c + 1);
          if (c != blank && !((core.merged[p] >> k) & 1ull) && !cut(p, core.klp[k])) {
            am[u] = core.klp[k] + (c == core.last[cur][p] ? core.b[cur][p] : asc[p]);
            ext[u] = am[u] > kNegInfB;        // only finite, unmerged, non-blank extensions go to the scorer
            if (ext[u]) sc.issue(s, g, u, cur, p, k, c, am[u]);
          }
        }
      }
      sc.chain(s, g, cur, pp);
#pragma unroll
      for (int u = 0; u < kLmGroup; ++u) {
        const int j = j0 + u;
        if (j >= J) continue;
        float v = am[u];
        carry[j] = Scorer::kNoCarry;
        if (ext[u]) v = sc.finish(s, g, u, cur, pp[u], kk[u], core.kcls[kk[u]], am[u], &carry[j]);
        comp[j] = ((uint64_t)desc_bits(v) << 32) | ck[u];
        if (v > kNegInfB) valid |= 1ull << j;
      }
    }
    // (4) select the W best, (5) compact and order them, write the next beam: the core fields, then the scorer's
    uint64_t prefix, mask;
    beam_select<J>(core, comp, valid, W, tid, &prefix, &mask);
    const int nsel = beam_compact<J>(core, comp, valid, prefix, mask, W, tid,
                                     [&](uint32_t pos, int j) { Scorer::on_keep(s, pos, carry[j]); });
    const int nxt = cur ^ 1;
    if (tid < nsel) {
      const int rank = beam_rank(core, nsel, tid);
      const int i = core.surv_i[tid];
      if (i < nbeam) {
        beam_keep_entry(core, cur, nxt, rank, i);
        sc.keep_entry(s, cur, nxt, rank, i);
      } else {
        const int q = i - nbeam, p = q / nk, k = q - p * nk;
        const int c = core.kcls[k];
        int64_t frame = t;                  // the trie numbers its nodes by the utterance's frame, not the chunk's
        if constexpr (Mode::kStream) frame += t0;
        beam_new_entry(core, cur, nxt, rank, p, c, frame, W, trie);
        core.nb[nxt][rank] = core.klp[k] + (c == core.last[cur][p] ? core.b[cur][p] : asc[p]);
        sc.new_entry(s, cur, nxt, rank, p, k, c, tid);
      }
    }
    nbeam = nsel;
    cur = nxt;
    __syncthreads();
  }
  if constexpr (Mode::kStream) {
    // the state after this chunk, before the end phase below touches the record: the re-rank writes core.score, fin and the
    // cur ^ 1 halves of node / len, none of which a frame reads before writing it, but the image is taken first all the same.
    // A chunk of no frames leaves the image as it is (a stream that was never fed stays the empty prefix).
    if (ok && L > 0) stream_copy_lds<typename Scorer::Lds, true>(s, reinterpret_cast<char*>(hdr) + sizeof(StreamHeader), tid);
    __syncthreads();                        // every thread's header reads and image loads are behind it
    if (tid == 0) {
      if (ok) {
        hdr->t0 = t0 + (int)L; hdr->nbeam = nbeam; hdr->cur = cur; hdr->dropped = dropped;
        hdr->live = (live || L > 0) ? 1 : 0;
      }
      margs.n_frames[ub] = t0 + (int)L;
      margs.n_dropped[ub] = dropped;
    }
  }
  // end of utterance: the scorer's final values of each entry, re-ranked where its end term can change the order
  const bool have = ok && tid < nbeam;
  float out[Scorer::kOuts];
#pragma unroll
  for (int n = 0; n < Scorer::kOuts; ++n) out[n] = n < 2 ? kNegInfB : 0.f;      // an empty slot: scores -inf, bias_scores 0
  int src = cur;
  if constexpr (Scorer::kRerank) {
    if (have) sc.final_scores(s, cur, tid, out);
    src = beam_final_rerank(core, Scorer::fin(s), cur, ok ? nbeam : 0, tid, out);
  }
  beam_write_back(core, src, nbeam, n_best, Tout, trie, io.tokens + ub * (int64_t)n_best * Tout, io.n_tokens + ub * n_best, ok, tid);
  if (tid < n_best) {
    const int64_t o = ub * n_best + tid;
    if constexpr (Scorer::kRerank) {
#pragma unroll
      for (int n = 0; n < Scorer::kOuts; ++n)
        if (have) out[n] = Scorer::fin(s)[n][tid];
    } else {
      if (have) sc.final_scores(s, cur, tid, out);
    }
    io.scores[o] = out[0];
#pragma unroll
    for (int n = 1; n < Scorer::kOuts; ++n) sc.extra_out(n)[o] = out[n];
  }
}

// ------------------------------------------------------------------ host side -------------------------------------------
bool beam_shape_ok(int64_t B, int64_t T, int64_t C, int W, int topn) {
  return B >= 1 && T >= 1 && C >= 1 && C <= kBeamMaxClasses && W >= 1 && W <= kBeamMaxWidth && topn >= 1 &&
         topn <= kBeamMaxTopN && B * T <= 0x7fffffffLL && 1 + T * (int64_t)W <= 0x7fffffffLL;
}

struct BeamWs {
  size_t kcls, klp, kn, trie, total;
};

BeamWs beam_ws(int64_t B, int64_t T, int64_t W) {
  BeamWs w;
  const size_t frames = (size_t)(B * T);
  w.kcls = 0;
  w.klp = align_up(w.kcls + frames * kBeamMaxTopN * sizeof(int32_t), 256);
  w.kn = align_up(w.klp + frames * kBeamMaxTopN * sizeof(float), 256);
  w.trie = align_up(w.kn + frames * sizeof(int32_t), 256);
  w.total = align_up(w.trie + (size_t)B * (size_t)(1 + T * W) * sizeof(int2), 256);
  return w;
}

// the arguments every decoder takes, as `who` (the exported function) received them
struct BeamArgs {
  const char* who;
  const float* logp;
  const int32_t* lens;
  int64_t B, T, C;
  int blank, beam_width, cutoff_top_n;
  float cutoff_prob;
  int n_best;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// the value checks every decoder makes; ptrs_ok: every pointer the caller requires is set
int beam_check_args(const BeamArgs& a, bool ptrs_ok) {
  LASR_CHECK_ARG(ptrs_ok, "%s: null pointer", a.who);
  LASR_CHECK_ARG(a.n_best >= 1 && a.n_best <= a.beam_width, "%s: n_best %d outside [1, beam_width %d]", a.who, a.n_best,
                 a.beam_width);
  LASR_CHECK_ARG(a.cutoff_prob > 0.f && a.cutoff_prob <= 1.f, "%s: cutoff_prob %g outside (0, 1]", a.who, (double)a.cutoff_prob);
  LASR_CHECK_ARG(a.C >= 1 && a.blank >= 0 && a.blank < a.C, "%s: blank %d outside [0, C = %lld)", a.who, a.blank, (long long)a.C);
  return 0;
}

// Checks the shape and the workspace, carves it, launches the prune kernel and then search(J, grid, stream, kc, kl, kn, trie)
// with J, the candidates per thread, as a std::integral_constant: the caller launches its kernel's instantiation.
// own_trie: the trie is the caller's (a stream's state holds it); the workspace is then the kept lists alone and `trie` null.
template <class Search>
int beam_launch(const BeamArgs& a, const char* search_name, Search search, bool own_trie = false) {
  LASR_CHECK_SHAPE(beam_shape_ok(a.B, a.T, a.C, a.beam_width, a.cutoff_top_n),
                   "%s: B %lld T %lld C %lld beam_width %d cutoff_top_n %d outside the supported range "
                   "(C <= %d, beam_width 1..%d, cutoff_top_n 1..%d)", a.who, (long long)a.B, (long long)a.T, (long long)a.C,
                   a.beam_width, a.cutoff_top_n, kBeamMaxClasses, kBeamMaxWidth, kBeamMaxTopN);
  const BeamWs w = beam_ws(a.B, a.T, a.beam_width);
  const size_t need = own_trie ? w.trie : w.total;
  if (a.workspace_bytes < need)
    return fail(LASR_E_WORKSPACE, "%s: workspace %zu < %zu bytes", a.who, a.workspace_bytes, need);
  char* ws = static_cast<char*>(a.workspace);
  int32_t* kc = reinterpret_cast<int32_t*>(ws + w.kcls);
  float* kl = reinterpret_cast<float*>(ws + w.klp);
  int32_t* kn = reinterpret_cast<int32_t*>(ws + w.kn);
  int2* trie = own_trie ? nullptr : reinterpret_cast<int2*>(ws + w.trie);
  hipStream_t st = as_stream(a.stream);
  hipLaunchKernelGGL(beam_prune_kernel, dim3((unsigned)(a.B * a.T)), dim3(64), 0, st, a.logp, a.lens, a.T, (int)a.C,
                     a.cutoff_top_n, a.cutoff_prob, kc, kl, kn);
  LASR_LAUNCH_CHECK("beam_prune_kernel");
  // candidates per frame: beam_width "no new label" entries + beam_width * kept labels, J per thread
  const int K = (int)(a.C < a.cutoff_top_n ? a.C : a.cutoff_top_n);
  const int per = (int)cdiv((int64_t)a.beam_width * (K + 1), kSearchThreads);
  const dim3 grid((unsigned)a.B);
  if (per <= 1) search(std::integral_constant<int, 1>{}, grid, st, kc, kl, kn, trie);
  else if (per <= 2) search(std::integral_constant<int, 2>{}, grid, st, kc, kl, kn, trie);
  else if (per <= 4) search(std::integral_constant<int, 4>{}, grid, st, kc, kl, kn, trie);
  else if (per <= 8) search(std::integral_constant<int, 8>{}, grid, st, kc, kl, kn, trie);
  else if (per <= 16) search(std::integral_constant<int, 16>{}, grid, st, kc, kl, kn, trie);
  else search(std::integral_constant<int, 33>{}, grid, st, kc, kl, kn, trie);
  LASR_LAUNCH_CHECK(search_name);
  return 0;
}

// What every exported decoder does after packing its arguments: the checks, then the two launches with Scorer's search.
template <class Scorer>
int beam_decode(const BeamArgs& a, const typename Scorer::Args& sargs, int32_t* tokens, int32_t* n_tokens, float* scores) {
  LASR_TRY(beam_check_args(a, a.logp && tokens && n_tokens && scores && a.workspace && Scorer::args_set(sargs)));
  if constexpr (std::is_same_v<typename Scorer::Args, LmArgs>)
    LASR_CHECK_ARG(std::isfinite(sargs.alpha) && std::isfinite(sargs.beta), "%s: alpha %g / beta %g not finite", a.who,
                   (double)sargs.alpha, (double)sargs.beta);
  return beam_launch(a, Scorer::kName, [&](auto j, dim3 grid, hipStream_t st, int32_t* kc, float* kl, int32_t* kn, int2* trie) {
    const BeamIo io{a.lens, a.T, (int)a.C, a.blank, a.beam_width, a.n_best, trie, tokens, n_tokens, scores};
    hipLaunchKernelGGL((beam_search_kernel<decltype(j)::value, Scorer>), grid, dim3(kSearchThreads), 0, st, kc, kl, kn, io, sargs,
                       OneShot::Args{});
  });
}

// ------------------------------------------------------------------ host side: streams ---------------------------------
// A stream's share of the caller's state buffer: header, LDS image of the kind's scorer, trie of T_cap frames.
struct StreamLayout {
  size_t trie, stride;
};

size_t stream_lds_bytes(int kind) {
  switch (kind) {
    case LASR_BEAM_PLAIN: return sizeof(NullScorer::Lds);
    case LASR_BEAM_LM: return sizeof(LmScorer<false>::Lds);
    case LASR_BEAM_WLM: return sizeof(WlmScorer::Lds);
    case LASR_BEAM_BIAS: return sizeof(BiasScorer::Lds);
    case LASR_BEAM_LM_BIAS: return sizeof(LmScorer<true>::Lds);
    default: return 0;
  }
}

bool stream_shape_ok(int64_t B, int64_t T_cap, int W, int kind) {
  return stream_lds_bytes(kind) != 0 && beam_shape_ok(B, T_cap, 1, W, 1);
}

StreamLayout stream_layout(int64_t T_cap, int W, int kind) {
  StreamLayout l;
  l.trie = align_up(sizeof(StreamHeader) + stream_lds_bytes(kind), 256);
  l.stride = align_up(l.trie + (size_t)(1 + T_cap * (int64_t)W) * sizeof(int2), 256);
  return l;
}

__global__ void beam_stream_reset_kernel(char* state, size_t stride, int64_t B, const int32_t* __restrict__ rows, int n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t b = rows ? (int64_t)rows[i] : i;
  if (b < 0 || b >= B) return;              // a row outside the buffer resets nothing
  StreamHeader* h = reinterpret_cast<StreamHeader*>(state + (size_t)b * stride);
  h->t0 = 0; h->nbeam = 1; h->cur = 0; h->dropped = 0; h->live = 0;
}

// what lasr_ctc_beam_stream_feed does once the kind has chosen Scorer: beam_decode's checks with the stream's own, then the
// prune launch over the chunk and the Streamed search
template <class Scorer>
int beam_stream_feed(const BeamArgs& a, const typename Scorer::Args& sargs, void* state, size_t state_bytes, int64_t T_cap, int kind,
                     int32_t* tokens, int32_t* n_tokens, float* scores, int32_t* n_frames, int32_t* n_dropped) {
  LASR_TRY(beam_check_args(a, a.logp && tokens && n_tokens && scores && n_frames && n_dropped && state && a.workspace &&
                                  Scorer::args_set(sargs)));
  if constexpr (std::is_same_v<typename Scorer::Args, LmArgs>)
    LASR_CHECK_ARG(std::isfinite(sargs.alpha) && std::isfinite(sargs.beta), "%s: alpha %g / beta %g not finite", a.who,
                   (double)sargs.alpha, (double)sargs.beta);
  LASR_CHECK_SHAPE(stream_shape_ok(a.B, T_cap, a.beam_width, kind),
                   "%s: B %lld T_cap %lld beam_width %d outside the supported range (beam_width 1..%d, 1 + T_cap * beam_width < 2^31)",
                   a.who, (long long)a.B, (long long)T_cap, a.beam_width, kBeamMaxWidth);
  const StreamLayout l = stream_layout(T_cap, a.beam_width, kind);
  if (state_bytes < (size_t)a.B * l.stride)
    return fail(LASR_E_WORKSPACE, "%s: state %zu < %zu bytes", a.who, state_bytes, (size_t)a.B * l.stride);
  return beam_launch(a, Scorer::kName, [&](auto j, dim3 grid, hipStream_t st, int32_t* kc, float* kl, int32_t* kn, int2*) {
    const BeamIo io{a.lens, a.T, (int)a.C, a.blank, a.beam_width, a.n_best, nullptr, tokens, n_tokens, scores};
    const Streamed::Args m{static_cast<char*>(state), l.stride, l.trie, T_cap, n_frames, n_dropped};
    hipLaunchKernelGGL((beam_search_kernel<decltype(j)::value, Scorer, Streamed>), grid, dim3(kSearchThreads), 0, st, kc, kl, kn, io,
                       sargs, m);
  }, true);
}

struct ArpaHandle {
  host::ArpaModel m;
};

int arpa_code(int rc) {
  switch (rc) {
    case host::kArpaErrFormat: return LASR_E_FORMAT;
    case host::kArpaErrUnsupported: return LASR_E_UNSUPPORTED;
    case host::kArpaErrOpen: return LASR_E_IO;
    default: return LASR_E_ARG;
  }
}

struct HotwordHandle {
  host::HotwordBank b;
};

}  // namespace
}  // namespace lasr

using namespace lasr;

// ------------------------------------------------------------------ the C ABI: decoders ---------------------------------
extern "C" size_t lasr_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t C, int beam_width, int cutoff_top_n) {
  if (!beam_shape_ok(B, T, C, beam_width, cutoff_top_n)) return 0;
  return beam_ws(B, T, beam_width).total;
}

extern "C" size_t lasr_ctc_beam_lm_workspace_bytes(int64_t B, int64_t T, int64_t C, int beam_width, int cutoff_top_n) {
  return lasr_ctc_beam_workspace_bytes(B, T, C, beam_width, cutoff_top_n);   // a scorer's own state is all in LDS
}

extern "C" int lasr_ctc_beam_decode(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                    int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, int32_t* tokens,
                                    int32_t* n_tokens, float* scores, void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a{"lasr_ctc_beam_decode", logp, lens, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, workspace,
                   workspace_bytes, stream};
  return beam_decode<NullScorer>(a, {}, tokens, n_tokens, scores);
}

extern "C" int lasr_ctc_beam_decode_lm(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                       int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, const void* lm_image,
                                       float alpha, float beta, int32_t* tokens, int32_t* n_tokens, float* scores,
                                       float* am_scores, void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a{"lasr_ctc_beam_decode_lm", logp, lens, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, workspace,
                   workspace_bytes, stream};
  return beam_decode<LmScorer<false>>(a, {logp, lm_image, alpha, beta, am_scores, nullptr, nullptr}, tokens, n_tokens, scores);
}

extern "C" int lasr_ctc_beam_decode_wlm(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                        int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, const void* lm_image,
                                        float alpha, float beta, int32_t* tokens, int32_t* n_tokens, float* scores,
                                        float* am_scores, void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a{"lasr_ctc_beam_decode_wlm", logp, lens, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, workspace,
                   workspace_bytes, stream};
  return beam_decode<WlmScorer>(a, {logp, lm_image, alpha, beta, am_scores, nullptr, nullptr}, tokens, n_tokens, scores);
}

extern "C" int lasr_ctc_beam_decode_bias(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                         int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, const void* bias_image,
                                         int32_t* tokens, int32_t* n_tokens, float* scores, float* am_scores, float* bias_scores,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a{"lasr_ctc_beam_decode_bias", logp, lens, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, workspace,
                   workspace_bytes, stream};
  return beam_decode<BiasScorer>(a, {bias_image, am_scores, bias_scores}, tokens, n_tokens, scores);
}

extern "C" int lasr_ctc_beam_decode_lm_bias(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                            int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, const void* lm_image,
                                            float alpha, float beta, const void* bias_image, int32_t* tokens, int32_t* n_tokens,
                                            float* scores, float* am_scores, float* bias_scores, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  const BeamArgs a{"lasr_ctc_beam_decode_lm_bias", logp, lens, B, T, C, blank, beam_width, cutoff_top_n, cutoff_prob, n_best, workspace,
                   workspace_bytes, stream};
  return beam_decode<LmScorer<true>>(a, {logp, lm_image, alpha, beta, am_scores, bias_image, bias_scores}, tokens, n_tokens, scores);
}

// ------------------------------------------------------------------ the C ABI: resumable search ------------------------
extern "C" size_t lasr_ctc_beam_stream_state_bytes(int64_t B, int64_t T_cap, int beam_width, int kind) {
  if (!stream_shape_ok(B, T_cap, beam_width, kind)) return 0;
  return (size_t)B * stream_layout(T_cap, beam_width, kind).stride;
}

extern "C" size_t lasr_ctc_beam_stream_workspace_bytes(int64_t B, int64_t T_chunk, int64_t C, int beam_width, int cutoff_top_n) {
  if (!beam_shape_ok(B, T_chunk, C, beam_width, cutoff_top_n)) return 0;
  return beam_ws(B, T_chunk, beam_width).trie;      // the kept lists of one chunk; the trie is part of the state
}

extern "C" int lasr_ctc_beam_stream_reset(void* state, size_t state_bytes, int64_t B, int64_t T_cap, int beam_width, int kind,
                                          const int32_t* rows, int n_rows, void* stream) {
  const char* who = "lasr_ctc_beam_stream_reset";
  LASR_CHECK_ARG(state, "%s: null pointer", who);
  LASR_CHECK_ARG(n_rows >= 0 && (rows || n_rows == 0), "%s: n_rows %d without rows, or negative", who, n_rows);
  LASR_CHECK_SHAPE(stream_shape_ok(B, T_cap, beam_width, kind),
                   "%s: B %lld T_cap %lld beam_width %d kind %d outside the supported range (beam_width 1..%d, 1 + T_cap * "
                   "beam_width < 2^31, kind 0..4)", who, (long long)B, (long long)T_cap, beam_width, kind, kBeamMaxWidth);
  const StreamLayout l = stream_layout(T_cap, beam_width, kind);
  if (state_bytes < (size_t)B * l.stride)
    return fail(LASR_E_WORKSPACE, "%s: state %zu < %zu bytes", who, state_bytes, (size_t)B * l.stride);
  const int n = rows ? n_rows : (int)B;
  if (n == 0) return 0;
  hipLaunchKernelGGL(beam_stream_reset_kernel, dim3((unsigned)cdiv((int64_t)n, 256)), dim3(256), 0, as_stream(stream),
                     static_cast<char*>(state), l.stride, B, rows, n);
  LASR_LAUNCH_CHECK("beam_stream_reset_kernel");
  return 0;
}

extern "C" int lasr_ctc_beam_stream_feed(const float* logp, const int32_t* lens, int64_t B, int64_t T_chunk, int64_t C, int blank,
                                         int beam_width, int cutoff_top_n, float cutoff_prob, int n_best,
                                         const lasr_beam_scorer* scorer, void* state, size_t state_bytes, int64_t T_cap,
                                         int32_t* tokens, int32_t* n_tokens, float* scores, int32_t* n_frames, int32_t* n_dropped,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const BeamArgs a{"lasr_ctc_beam_stream_feed", logp, lens, B, T_chunk, C, blank, beam_width, cutoff_top_n, cutoff_prob, n_best,
                   workspace, workspace_bytes, stream};
  LASR_CHECK_ARG(scorer, "%s: null pointer", a.who);
  const lasr_beam_scorer& s = *scorer;
  const LmArgs lm{logp, s.lm_image, s.alpha, s.beta, s.am_scores, s.bias_image, s.bias_scores};
  switch (s.kind) {
    case LASR_BEAM_PLAIN:
      return beam_stream_feed<NullScorer>(a, {}, state, state_bytes, T_cap, s.kind, tokens, n_tokens, scores, n_frames, n_dropped);
    case LASR_BEAM_LM:
      return beam_stream_feed<LmScorer<false>>(a, lm, state, state_bytes, T_cap, s.kind, tokens, n_tokens, scores, n_frames, n_dropped);
    case LASR_BEAM_WLM:
      return beam_stream_feed<WlmScorer>(a, lm, state, state_bytes, T_cap, s.kind, tokens, n_tokens, scores, n_frames, n_dropped);
    case LASR_BEAM_BIAS:
      return beam_stream_feed<BiasScorer>(a, {s.bias_image, s.am_scores, s.bias_scores}, state, state_bytes, T_cap, s.kind, tokens,
                                          n_tokens, scores, n_frames, n_dropped);
    case LASR_BEAM_LM_BIAS:
      return beam_stream_feed<LmScorer<true>>(a, lm, state, state_bytes, T_cap, s.kind, tokens, n_tokens, scores, n_frames, n_dropped);
    default:
      return fail(LASR_E_ARG, "%s: scorer kind %d outside 0..4", a.who, s.kind);
  }
}

// ------------------------------------------------------------------ the C ABI: ARPA models ------------------------------
extern "C" int lasr_arpa_load(const char* path, const char* const* vocab, int n_vocab, void** handle) {
  LASR_CHECK_ARG(path && handle && (vocab || n_vocab == 0) && n_vocab >= 0, "lasr_arpa_load: null pointer or negative n_vocab");
  *handle = nullptr;
  ArpaHandle* h = new ArpaHandle();
  std::string err;
  const int rc = host::arpa_load(path, vocab, n_vocab, &h->m, &err);   // arpa_io.h (also built under ASan / UBSan)
  if (rc != host::kArpaOk) {
    delete h;
    return fail(arpa_code(rc), "lasr_arpa_load: %s", err.c_str());
  }
  *handle = h;
  return 0;
}

extern "C" int lasr_arpa_load_words(const char* path, const char* const* vocab, int n_vocab, int space_id, void** handle) {
  LASR_CHECK_ARG(path && handle && (vocab || n_vocab == 0) && n_vocab >= 0,
                 "lasr_arpa_load_words: null pointer or negative n_vocab");
  *handle = nullptr;
  ArpaHandle* h = new ArpaHandle();
  std::string err;
  const int rc = host::arpa_load_words(path, vocab, n_vocab, space_id, &h->m, &err);   // arpa_io.h, as lasr_arpa_load
  if (rc != host::kArpaOk) {
    delete h;
    return fail(arpa_code(rc), "lasr_arpa_load_words: %s", err.c_str());
  }
  *handle = h;
  return 0;
}

extern "C" int lasr_arpa_info(const void* handle, int* order, int* char_based, int64_t* n_ngrams, size_t* image_bytes) {
  LASR_CHECK_ARG(handle, "lasr_arpa_info: null handle");
  const host::ArpaModel& m = static_cast<const ArpaHandle*>(handle)->m;
  if (order) *order = m.order;
  if (char_based) *char_based = m.char_based ? 1 : 0;
  if (n_ngrams) *n_ngrams = m.n_ngrams;
  if (image_bytes) *image_bytes = m.image.size();
  return 0;
}

extern "C" int lasr_arpa_lexicon_info(const void* handle, int64_t* n_lexicon_words, int64_t* n_nodes, int64_t* n_dropped_words) {
  LASR_CHECK_ARG(handle, "lasr_arpa_lexicon_info: null handle");
  const host::ArpaModel& m = static_cast<const ArpaHandle*>(handle)->m;
  LASR_CHECK_ARG(m.word_mode, "lasr_arpa_lexicon_info: the handle is not one of lasr_arpa_load_words");
  if (n_lexicon_words) *n_lexicon_words = m.n_lexicon_words;
  if (n_nodes) *n_nodes = m.n_nodes;
  if (n_dropped_words) *n_dropped_words = m.n_dropped_words;
  return 0;
}

extern "C" int lasr_arpa_write_image(const void* handle, void* host_dst, size_t bytes) {
  LASR_CHECK_ARG(handle && host_dst, "lasr_arpa_write_image: null pointer");
  const host::ArpaModel& m = static_cast<const ArpaHandle*>(handle)->m;
  if (bytes < m.image.size())
    return fail(LASR_E_WORKSPACE, "lasr_arpa_write_image: %zu < %zu bytes", bytes, m.image.size());
  memcpy(host_dst, m.image.data(), m.image.size());
  return 0;
}

extern "C" void lasr_arpa_free(void* handle) { delete static_cast<ArpaHandle*>(handle); }

// ------------------------------------------------------------------ the C ABI: hotword banks ----------------------------
extern "C" int lasr_hotword_build(const int32_t* labels, const int64_t* offsets, const float* weights, int n_phrases, int64_t C,
                                  int blank, void** handle) {
  LASR_CHECK_ARG(handle, "lasr_hotword_build: null handle");
  *handle = nullptr;
  HotwordHandle* h = new HotwordHandle();
  std::string err;
  const int rc = host::hotword_build(labels, offsets, weights, n_phrases, C, blank, &h->b, &err);   // hotword_io.h (also built
  if (rc != host::kHotwordOk) {                                                                      // under ASan / UBSan)
    delete h;
    return fail(rc == host::kHotwordErrFormat ? LASR_E_FORMAT : LASR_E_ARG, "lasr_hotword_build: %s", err.c_str());
  }
  *handle = h;
  return 0;
}

extern "C" int lasr_hotword_info(const void* handle, int64_t* n_phrases, int64_t* n_nodes, float* max_credit, size_t* image_bytes) {
  LASR_CHECK_ARG(handle, "lasr_hotword_info: null handle");
  const host::HotwordBank& b = static_cast<const HotwordHandle*>(handle)->b;
  if (n_phrases) *n_phrases = b.n_phrases;
  if (n_nodes) *n_nodes = b.n_nodes;
  if (max_credit) *max_credit = b.max_credit;
  if (image_bytes) *image_bytes = b.image.size();
  return 0;
}

extern "C" int lasr_hotword_write_image(const void* handle, void* host_dst, size_t bytes) {
  LASR_CHECK_ARG(handle && host_dst, "lasr_hotword_write_image: null pointer");
  const host::HotwordBank& b = static_cast<const HotwordHandle*>(handle)->b;
  if (bytes < b.image.size())
    return fail(LASR_E_WORKSPACE, "lasr_hotword_write_image: %zu < %zu bytes", bytes, b.image.size());
  memcpy(host_dst, b.image.data(), b.image.size());
  return 0;
}

extern "C" void lasr_hotword_free(void* handle) { delete static_cast<HotwordHandle*>(handle); }

extern "C" int lasr_hotword_score(const void* handle, const int32_t* labels, int64_t n, float* bonus, float* final_bonus,
                                  int32_t* state) {
  LASR_CHECK_ARG(handle && (labels || n == 0) && n >= 0, "lasr_hotword_score: null pointer or negative length");
  const host::HotwordBank& b = static_cast<const HotwordHandle*>(handle)->b;
  std::string err;
  const int rc = host::hotword_score(b.image.data(), b.image.size(), labels, n, bonus, final_bonus, state, &err);
  if (rc != host::kHotwordOk) return fail(rc == host::kHotwordErrFormat ? LASR_E_FORMAT : LASR_E_ARG, "lasr_hotword_score: %s", err.c_str());
  return 0;
}
