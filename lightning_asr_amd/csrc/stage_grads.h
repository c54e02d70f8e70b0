// The gradients a backward stage defers to its end: 1x1 weight-gradient problems waiting for ONE split-K launch, and finished
// partial sums waiting for ONE reduction.  Host code over include/lasr.h alone (tests/sanitize/stage_grads_check.cpp drives it with
// a recording launcher); model.hip gives it the two real launches.
//
// How problems are grouped into launches decides each launch's slice count, and so the bits of the gradients: the rules below are
// the flush points of the step, not a tuning knob.
#pragma once
#include "../../include/lasr.h"
#include <vector>

namespace lasr {

int fail(int code, const char* fmt, ...);   // the library's error reporter (common.h)

// Launch supplies the two launches and the capacities of their kernels' argument structs:
//   static constexpr int kMaxProblems, kMaxSegments;
//   int wgrads(probs, n, slabs, splits, riders, n_riders, &riders_taken);   splits[i] slabs of M*N floats are left in slabs[i]; the
//                                                                          first riders_taken of `riders` were reduced by the launch
//   int reduce(descs, n, closing);                                         closing: the stage's last reduction
template <class Launch>
struct StageGrads {
  // What joins between two relieve() calls: a unit without a depthwise conv (one problem, and no relieve() of its own) and a
  // depthwise unit (two problems, one segment of depthwise partials).
  static constexpr int kUnitProblems = 3, kUnitReductions = 1;
  // a full launch's problems all become segments of one reduction, with room for what a unit adds before relieve() looks again
  static_assert(Launch::kMaxProblems + kUnitProblems + kUnitReductions <= Launch::kMaxSegments, "a flush must fit one reduction");

  Launch launch;
  std::vector<lasr_reduce_desc> pending;   // finished partial sums, in the order they were added
  std::vector<lasr_gemm_problem> probs;    // weight-gradient problems not launched yet, and the slab buffer of each
  std::vector<float*> slabs;

  explicit StageGrads(const Launch& l) : launch(l) {}

  // THE invariant: whatever is in flight fits one reduction, because every problem becomes a segment when it is flushed.
  int check() const {
    if (pending.size() + probs.size() > (size_t)Launch::kMaxSegments)
      return fail(LASR_E_ARG, "StageGrads: %zu segments + %zu problems in flight, a reduction takes %d", pending.size(), probs.size(),
                  Launch::kMaxSegments);
    return 0;
  }

  // a unit's one or two 1x1 weight gradients; a pair is never split across launches
  int add_wgrads(const lasr_gemm_problem* pr, int n, float* const* slab) {
    if (probs.size() + n > (size_t)Launch::kMaxProblems) {
      int rc = flush();
      if (rc) return rc;
    }
    for (int i = 0; i < n; ++i) { probs.push_back(pr[i]); slabs.push_back(slab[i]); }
    return check();
  }
  // partial sums that are complete once the launches issued so far have run (depthwise dW, the BiLSTM's dW_hh and bias sums)
  int add_reduction(const lasr_reduce_desc& d) {
    pending.push_back(d);
    return check();
  }
  // the first n problems were launched in splits[i] slices: their slabs are segments now (the one slab -> segment conversion)
  void retire(int n, const int* splits) {
    for (int i = 0; i < n; ++i) pending.push_back({slabs[i], reinterpret_cast<float*>(probs[i].C), probs[i].M * probs[i].N, splits[i]});
    probs.erase(probs.begin(), probs.begin() + n);
    slabs.erase(slabs.begin(), slabs.begin() + n);
  }
  // The problems collected so far as ONE split-K launch.  Whatever `pending` holds is complete and is offered as riders: the launch
  // reduces as many of them, from the front, as its idle CUs have time for, and those leave the list.  Same sums, same order.
  int flush() {
    if (probs.empty()) return 0;
    int splits[Launch::kMaxProblems], taken = 0;
    int rc = launch.wgrads(probs.data(), (int)probs.size(), slabs.data(), splits, pending.data(), (int)pending.size(), &taken);
    if (rc) return rc;
    if (taken > 0) pending.erase(pending.begin(), pending.begin() + taken);
    retire((int)probs.size(), splits);
    return 0;
  }
  // Make room for `extra_reductions` segments and `extra_problems` problems that are about to join: when they would not fit, launch
  // and reduce what is there.
  int relieve(int extra_reductions = kUnitReductions, int extra_problems = kUnitProblems) {
    if (pending.size() + probs.size() + extra_reductions + extra_problems <= (size_t)Launch::kMaxSegments) return 0;
    int rc = flush();
    if (!rc) rc = launch.reduce(pending.data(), (int)pending.size(), false);
    pending.clear();
    return rc;
  }
  // the end of the stage: after this its gradients are final
  int close() {
    int rc = flush();
    if (!rc && !pending.empty()) rc = launch.reduce(pending.data(), (int)pending.size(), true);
    pending.clear();
    return rc;
  }
};

}  // namespace lasr
