// CPU sanitizer pass over the collector of a backward stage's deferred gradients: built by tests/test_sanitize_stage_grads_cpu.py as
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/sanitize/stage_grads_check.cpp
// against lightning_asr_amd/csrc/stage_grads.h - the SAME source model.hip compiles.  No GPU, no HIP.  A recording launcher stands in
// for the split-K weight-gradient launch and for lasr_reduce_many, and drives the collector through what the shipped models never
// reach:
//   1. 31 problems followed by a pair; 33 single problems;
//   2. more than 60 entries from depthwise-style units (a pair, one segment, relieve());
//   3. the context join (six segments, two problems) arriving at 55, 56 and 57 entries;
//   4. a launcher that takes no, some or all riders; retire() of 0, k and all problems;
//   5. more entries than a reduction takes without a relieve(): an error code, no abort;
//   6. the plain model's 15 units and the context model's 16, as one stage and as the staged calls' buckets: the launches the step
//      makes for them (profiles/stage_collector_reduce_dump_parent.txt).
// After every step the in-flight total is within a reduction's capacity; after close() every problem was launched once, every segment
// reduced once with its launch's slice count and in the order it became one, no pair was split and nothing is left.
#include "../../lightning_asr_amd/csrc/stage_grads.h"

#include <cstdarg>
#include <cstdio>
#include <map>
#include <utility>

static int g_fail = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

static int g_errors = 0;   // lasr::fail calls
int lasr::fail(int code, const char*, ...) { ++g_errors; return code; }

enum Riders { kNone, kSome, kAll };

struct Flush { std::vector<const void*> outs; int offered, taken; };
struct Reduction { std::vector<lasr_reduce_desc> segs; bool closing; };
struct Log {
  Riders policy = kNone;
  std::vector<Flush> flushes;
  std::vector<Reduction> reductions;
  std::vector<const float*> became, reduced;   // segments in the order they came to exist / were reduced (riders included)
  std::map<const float*, int> slices;          // slab -> slice count of its launch
};

struct Recorder {
  static constexpr int kMaxProblems = 32, kMaxSegments = 64, kMaxRiders = 24;
  Log* log;
  int wgrads(const lasr_gemm_problem* probs, int n, float* const* slabs, int* splits, const lasr_reduce_desc* riders, int n_riders, int* taken) const {
    CHECK(n >= 1 && n <= kMaxProblems, "launch of %d problems", n);
    CHECK(n_riders >= 0 && n_riders <= kMaxSegments, "%d riders offered", n_riders);
    const int most = n_riders < kMaxRiders ? n_riders : kMaxRiders;
    *taken = log->policy == kNone ? 0 : log->policy == kSome ? most / 2 : most;
    for (int i = 0; i < *taken; ++i) {
      log->reduced.push_back(riders[i].partials);
      if (log->slices.count(riders[i].partials)) CHECK(riders[i].n_partials == log->slices[riders[i].partials], "a rider's slice count");
    }
    Flush f;
    f.offered = n_riders; f.taken = *taken;
    const int split = 2 + (int)log->flushes.size();   // every launch its own slice count
    for (int i = 0; i < n; ++i) {
      splits[i] = split;
      f.outs.push_back(probs[i].C);
      log->became.push_back(slabs[i]);
      CHECK(!log->slices.count(slabs[i]), "a problem was launched twice");
      log->slices[slabs[i]] = split;
    }
    log->flushes.push_back(f);
    return 0;
  }
  int reduce(const lasr_reduce_desc* d, int n, bool closing) const {
    CHECK(n >= 1 && n <= kMaxSegments, "reduction of %d segments", n);
    Reduction r;
    r.closing = closing;
    for (int i = 0; i < n; ++i) { r.segs.push_back(d[i]); log->reduced.push_back(d[i].partials); }
    log->reductions.push_back(r);
    return 0;
  }
};
using Stage = lasr::StageGrads<Recorder>;

// One stage under test: hands out distinct fake addresses (never read), and keeps what was added.
struct Bench {
  Log log;
  Stage sg;
  std::vector<const void*> added;                       // problems' outputs, in the order they were added
  std::vector<std::pair<const void*, const void*>> pairs;
  float arena[4096];
  int next = 0;
  explicit Bench(Riders policy) : sg(Recorder{&log}) { log.policy = policy; }
  float* fresh() { return &arena[next++]; }
  void inflight() { CHECK(sg.pending.size() + sg.probs.size() <= (size_t)Recorder::kMaxSegments, "%zu + %zu in flight", sg.pending.size(), sg.probs.size()); }
  int wgrads(int n, int64_t elems) {
    lasr_gemm_problem pr[2] = {};
    float* slab[2] = {nullptr, nullptr};
    for (int i = 0; i < n; ++i) { pr[i].C = fresh(); pr[i].M = elems; pr[i].N = 1; pr[i].K = 1; slab[i] = fresh(); added.push_back(pr[i].C); }
    if (n == 2) pairs.push_back({pr[0].C, pr[1].C});
    const int rc = sg.add_wgrads(pr, n, slab);
    inflight();
    return rc;
  }
  int reduction(int64_t elems) {
    const float* part = fresh();
    log.became.push_back(part);
    const int rc = sg.add_reduction({part, fresh(), elems, 5});
    inflight();
    return rc;
  }
  int relieve() { const int rc = sg.relieve(); inflight(); return rc; }
  int relieve(int r, int p) { const int rc = sg.relieve(r, p); inflight(); return rc; }
  void retire(int n) {          // what the launch beside the recurrences leaves: the first n problems are slabs of 9 slices now
    int splits[Recorder::kMaxProblems];
    for (int i = 0; i < n; ++i) { splits[i] = 9; log.became.push_back(sg.slabs[i]); log.slices[sg.slabs[i]] = 9; }
    Flush f;
    f.offered = 0; f.taken = 0;
    for (int i = 0; i < n; ++i) f.outs.push_back(sg.probs[i].C);
    if (n) log.flushes.push_back(f);
    sg.retire(n, splits);
    inflight();
  }
  // a unit of the model: one or two 1x1 weight gradients, and for a depthwise unit its partials and the look at the capacity
  void unit(bool pair, bool dw, int64_t w_elems = 7, int64_t dw_elems = 3) {
    CHECK(wgrads(pair ? 2 : 1, w_elems) == 0, "add_wgrads");
    if (dw) { CHECK(reduction(dw_elems) == 0, "add_reduction"); CHECK(relieve() == 0, "relieve"); }
  }
  void finish(const char* what) {
    CHECK(sg.close() == 0, "%s: close", what);
    CHECK(sg.pending.empty() && sg.probs.empty() && sg.slabs.empty(), "%s: close() left something", what);
    std::vector<const void*> launched;
    std::map<const void*, int> where;
    for (size_t f = 0; f < log.flushes.size(); ++f) {
      CHECK(log.flushes[f].taken <= Recorder::kMaxRiders && log.flushes[f].taken <= log.flushes[f].offered, "%s: riders", what);
      for (const void* o : log.flushes[f].outs) { launched.push_back(o); where[o] = (int)f; }
    }
    CHECK(launched == added, "%s: %zu problems launched, %zu added, or another order", what, launched.size(), added.size());
    for (const auto& pr : pairs) CHECK(where[pr.first] == where[pr.second], "%s: a pair was split", what);
    CHECK(log.reduced == log.became, "%s: %zu segments reduced, %zu made, or another order", what, log.reduced.size(), log.became.size());
    for (const Reduction& r : log.reductions)
      for (const lasr_reduce_desc& d : r.segs)
        if (log.slices.count(d.partials)) CHECK(d.n_partials == log.slices[d.partials], "%s: slice count %d", what, d.n_partials);
    CHECK(g_errors == 0, "%s: %d errors reported", what, g_errors);
  }
  std::vector<size_t> flush_sizes() const { std::vector<size_t> v; for (const Flush& f : log.flushes) v.push_back(f.outs.size()); return v; }
  size_t riders_taken() const { size_t n = 0; for (const Flush& f : log.flushes) n += (size_t)f.taken; return n; }
  std::vector<size_t> reduce_sizes() const { std::vector<size_t> v; for (const Reduction& r : log.reductions) v.push_back(r.segs.size()); return v; }
};

static const Riders kPolicies[3] = {kNone, kSome, kAll};
using Sizes = std::vector<size_t>;

static void problem_limit() {
  for (Riders pol : kPolicies) {
    Bench a(pol);
    for (int i = 0; i < 31; ++i) a.unit(false, false);
    a.unit(true, false);                                   // 31 + 2: the pair waits for the next launch
    CHECK(a.flush_sizes() == Sizes({31}), "31 + pair: first launch");
    a.finish("31 + pair");
    CHECK(a.flush_sizes() == Sizes({31, 2}) && a.reduce_sizes() == Sizes({33 - a.riders_taken()}), "31 + pair");
    Bench b(pol);
    for (int i = 0; i < 33; ++i) b.unit(false, false);
    b.finish("33 singles");
    CHECK(b.flush_sizes() == Sizes({32, 1}) && b.reduce_sizes() == Sizes({33 - b.riders_taken()}), "33 singles");
  }
}

static void depthwise_units_past_60() {
  for (Riders pol : kPolicies) {
    Bench a(pol);
    for (int i = 0; i < 20; ++i) a.unit(true, true);       // 16 units filled a launch, the 17th flushed it with 16 riders on offer
    CHECK(a.flush_sizes() == Sizes({32}) && a.log.flushes[0].offered == 16 && a.reduce_sizes().empty(), "20 units");
    if (pol == kNone) {                                    // no rider left the list: 60 entries, and 63 > 60 with the next unit
      a.unit(true, true);
      CHECK(a.flush_sizes() == Sizes({32, 10}) && a.reduce_sizes() == Sizes({63}), "21 units: launch and reduce");
      CHECK(!a.log.reductions[0].closing && a.sg.pending.empty() && a.sg.probs.empty(), "21 units: relieved");
    }
    for (int i = 0; i < 30; ++i) a.unit(true, true);
    CHECK(!a.log.reductions.empty(), "50 units: relieved on the way");
    a.finish("50 depthwise units");
  }
}

static void context_join() {
  for (Riders pol : kPolicies)
    for (int at = 55; at <= 57; ++at) {
      Bench a(pol);
      for (int i = 0; i < 15; ++i) a.unit(true, false);    // 30 problems, then segments up to `at` entries
      for (int i = 30; i < at; ++i) CHECK(a.reduction(3) == 0, "add_reduction");
      CHECK(a.relieve(6, 2) == 0, "relieve(6, 2)");
      CHECK(a.log.reductions.size() == (at + 8 > 64 ? 1u : 0u), "join at %d: %zu reductions", at, a.log.reductions.size());
      for (int d = 0; d < 2; ++d) {
        for (int i = 0; i < 3; ++i) CHECK(a.reduction(3) == 0, "add_reduction");
        a.unit(false, false);
      }
      CHECK(a.relieve() == 0, "relieve");
      a.finish("context join");
      // 55: 63 entries after the join, over 60: relieved.  56: 64, the same.  57: relieved before the join, 8 entries after it.
      CHECK(a.reduce_sizes().size() == (at == 57 ? 2u : 1u), "join at %d: %zu reductions in all", at, a.reduce_sizes().size());
    }
}

static void retire_some() {
  for (int k : {0, 3, 10}) {
    Bench a(kAll);
    for (int i = 0; i < 5; ++i) a.unit(true, false);
    a.retire(k);
    CHECK(a.sg.pending.size() == (size_t)k && a.sg.probs.size() == (size_t)(10 - k), "retire(%d)", k);
    for (int i = 0; i < k; ++i) CHECK(a.sg.pending[i].n_partials == 9 && a.sg.pending[i].n == 7, "retire(%d): segment %d", k, i);
    a.pairs.clear();                                       // (the launch beside the recurrences takes what its budget allows: pairs may part)
    a.finish("retire");
  }
}

static void overflow_is_an_error() {
  Bench a(kNone);
  for (int i = 0; i < 64; ++i) CHECK(a.sg.add_reduction({a.fresh(), a.fresh(), 1, 1}) == 0, "segment %d", i);
  CHECK(g_errors == 0, "no error so far");
  CHECK(a.sg.add_reduction({a.fresh(), a.fresh(), 1, 1}) == LASR_E_ARG && g_errors == 1, "65 segments in flight: LASR_E_ARG");
  lasr_gemm_problem pr = {};
  float* slab = a.fresh();
  CHECK(a.sg.add_wgrads(&pr, 1, &slab) == LASR_E_ARG && g_errors == 2, "a problem on top: LASR_E_ARG");
  g_errors = 0;
}

// The models' units from the last to the first, as the backward walks them: {ci, co, k}; k = 0: no depthwise conv.
struct U { int ci, co, k; bool pair; };
static std::vector<U> model_units(bool ctx) {
  std::vector<U> u = {{512, 1024, 0, false}};
  if (ctx) u.push_back({512, 512, 87, true});
  const U blocks[13] = {{512, 512, 75, true}, {512, 512, 63, true}, {512, 512, 63, true}, {512, 512, 63, true}, {512, 512, 51, true},
                        {512, 512, 51, true}, {ctx ? 336 : 256, 512, 51, true}, {256, 256, 39, true}, {256, 256, 39, true},
                        {256, 256, 39, true}, {256, 256, 33, true}, {256, 256, 33, true}, {256, 256, 33, true}};
  for (const U& b : blocks) u.push_back(b);
  u.push_back({64, 256, 33, false});
  return u;
}
static std::vector<int64_t> seg_elems(const Reduction& r) { std::vector<int64_t> v; for (const lasr_reduce_desc& d : r.segs) v.push_back(d.n); return v; }

static void replay_models() {
  // plain, one stage: 28 problems in one launch that is offered the 14 depthwise segments; one reduction of what it left
  for (Riders pol : kPolicies) {
    Bench a(pol);
    for (const U& u : model_units(false)) a.unit(u.pair, u.k > 0, (int64_t)u.co * u.ci, (int64_t)u.ci * u.k);
    a.finish("plain");
    CHECK(a.flush_sizes() == Sizes({28}) && a.log.flushes[0].offered == 14, "plain: one launch of 28, 14 riders offered");
    CHECK(a.reduce_sizes() == Sizes({(size_t)(42 - a.log.flushes[0].taken)}) && a.log.reductions[0].closing, "plain: one reduction");
    if (pol == kNone)      // the golden inputs' step (no riders at that size): 42 segments
      CHECK(seg_elems(a.log.reductions[0]) == std::vector<int64_t>({38400, 32256, 32256, 32256, 26112, 26112, 13056, 9984, 9984, 9984, 8448, 8448, 8448, 2112,
                                                                     524288, 262144, 262144, 262144, 262144, 262144, 262144, 262144, 262144, 262144, 262144,
                                                                     262144, 262144, 131072, 131072, 65536, 65536, 65536, 65536, 65536, 65536, 65536, 65536,
                                                                     65536, 65536, 65536, 65536, 16384}), "plain: the 42 segments");
    if (pol == kAll) CHECK(a.reduce_sizes() == Sizes({28}), "plain, benchmark shapes: the launch takes all 14 riders, 28 segments are left");
  }
  // plain, the staged calls: 2 buckets end after block3 (22 + 20 segments), 4 buckets after last_cnn2, block3 and block1 (1, 21, 18, 2)
  const std::vector<std::vector<size_t>> cuts = {{8, 15}, {1, 8, 14, 15}};
  const std::vector<Sizes> want = {{22, 20}, {1, 21, 18, 2}};
  for (size_t c = 0; c < cuts.size(); ++c) {
    const std::vector<U> units = model_units(false);
    Sizes got;
    size_t lo = 0;
    for (size_t hi : cuts[c]) {
      Bench a(kNone);
      for (size_t i = lo; i < hi; ++i) a.unit(units[i].pair, units[i].k > 0);
      a.finish("plain, staged");
      CHECK(a.log.flushes.size() == 1 && a.log.reductions.size() == 1, "plain, staged: one launch and one reduction per stage");
      got.push_back(a.log.reductions[0].segs.size());
      lo = hi;
    }
    CHECK(got == want[c], "plain, staged: segments per stage");
  }
  // context, the separate form (the golden inputs' step): the BiLSTM's gradients do not pass through the collector
  {
    Bench a(kNone);
    for (const U& u : model_units(true)) a.unit(u.pair, u.k > 0);
    a.finish("context, separate");
    CHECK(a.flush_sizes() == Sizes({30}) && a.reduce_sizes() == Sizes({45}), "context, separate: 30 problems, 45 segments");
  }
  // context, beside the recurrences (benchmark shapes): that launch takes 15 of the 17 problems collected down to block3, the join adds
  // six segments and two problems, the closing launch has 17 problems and takes no rider, the reduction 53 segments
  {
    Bench a(kNone);
    const std::vector<U> units = model_units(true);
    for (size_t i = 0; i < units.size(); ++i) {
      a.unit(units[i].pair, units[i].k > 0, (int64_t)units[i].co * units[i].ci, (int64_t)units[i].ci * units[i].k);
      if (units[i].ci != 336) continue;
      CHECK(a.sg.probs.size() == 17 && a.sg.pending.size() == 8, "context: 17 problems and 8 segments at the branch");
      a.pairs.clear();
      a.retire(15);
      CHECK(a.relieve(6, 2) == 0 && a.log.reductions.empty(), "context: room for the join");
      for (int d = 0; d < 2; ++d) {
        CHECK(a.reduction(6400) == 0 && a.reduction(160) == 0 && a.reduction(160) == 0, "context: the BiLSTM's segments");
        CHECK(a.wgrads(1, 160 * 256) == 0, "context: dW_ih");
      }
      CHECK(a.relieve() == 0 && a.log.reductions.empty(), "context: no reduction at the join");
    }
    a.finish("context, beside");
    CHECK(a.flush_sizes() == Sizes({15, 17}) && a.log.flushes[1].offered == 36, "context: the closing launch");
    CHECK(a.reduce_sizes() == Sizes({53}), "context: 53 segments");
    CHECK(seg_elems(a.log.reductions[0]) == std::vector<int64_t>({44544, 38400, 32256, 32256, 32256, 26112, 26112, 17136, 524288, 262144, 262144, 262144, 262144,
                                                                   262144, 262144, 262144, 262144, 262144, 262144, 262144, 262144, 262144, 262144, 6400, 160,
                                                                   160, 6400, 160, 160, 9984, 9984, 9984, 8448, 8448, 8448, 2112, 172032, 172032, 40960, 40960,
                                                                   65536, 65536, 65536, 65536, 65536, 65536, 65536, 65536, 65536, 65536, 65536, 65536, 16384}),
          "context: the 53 segments");
  }
}

int main() {
  problem_limit();
  depthwise_units_past_60();
  context_join();
  retire_some();
  overflow_is_an_error();
  replay_models();
  if (g_fail) { fprintf(stderr, "stage_grads_check: %d failures\n", g_fail); return 1; }
  printf("stage_grads_check ok\n");
  return 0;
}
