"""Dev tool: time lasr_edit_align_batch against lasr_edit_distance_batch in one process at the validation shape of cfg2 (B=32,
references of ~100 labels, hypotheses in a (32, 501) token block), token units and word units, for two kinds of hypotheses: the
~T' tokens an untrained model emits, and a noisy copy of the reference (a trained model).  The two calls alternate in windows
of `reps` calls between device events; the figure is the median window.  Outputs and the workspace are allocated once.  Writes
profiles/edit_ops_time.json.
python tools/edit_ops_time.py [reps] [windows]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from lightning_asr_amd import _lib  # noqa: E402

B, T, S, C = 32, 501, 110, 28


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def make(kind, g):
    """(hyp (B,T) i32, hyp_lens, ref (B,S) i64, ref_lens): label 0 is the space, about one in six"""
    ref = torch.randint(1, C, (B, S), generator=g)
    ref[torch.rand(B, S, generator=g) < 1 / 6] = 0
    ref_lens = torch.randint(90, S + 1, (B,), generator=g).to(torch.int32)
    hyp = torch.randint(1, C, (B, T), generator=g)
    hyp[torch.rand(B, T, generator=g) < 1 / 6] = 0
    if kind == "untrained":
        hyp_lens = torch.randint(T - 100, T + 1, (B,), generator=g).to(torch.int32)
    else:                                   # the reference with one token in ten replaced
        hyp[:, :S] = torch.where(torch.rand(B, S, generator=g) < 0.1, hyp[:, :S], ref)
        hyp_lens = ref_lens.clone()
    return hyp.to(torch.int32), hyp_lens, ref, ref_lens


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    dev = torch.device("cuda")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = {"B": B, "hyp_pitch": T, "ref_pitch": S, "reps_per_window": reps, "windows": windows, "unit": "us per call, median window",
           "cases": {}}
    g = torch.Generator().manual_seed(1)
    nb = int(lib.lasr_edit_align_workspace_bytes(B, T, S))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    dist, units, n_ops = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    dist2, units2 = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
    script = torch.empty(B, T + S, dtype=torch.uint8, device=dev)
    for kind in ("untrained", "trained"):
        hyp, hyp_lens, ref, ref_lens = (t.to(dev).contiguous() for t in make(kind, g))
        for mode, space in (("tokens", -1), ("words", 0)):
            def distance():
                _lib.call("lasr_edit_distance_batch", hyp.data_ptr(), hyp_lens.data_ptr(), T, ref.data_ptr(), ref_lens.data_ptr(), S, B, space,
                          dist2.data_ptr(), units2.data_ptr(), None, st)

            def align():
                _lib.call("lasr_edit_align_batch", hyp.data_ptr(), hyp_lens.data_ptr(), T, ref.data_ptr(), ref_lens.data_ptr(), S, B, space,
                          dist.data_ptr(), units.data_ptr(), counts.data_ptr(), script.data_ptr(), T + S, n_ops.data_ptr(), None, None, 0,
                          ws.data_ptr(), nb, st)

            for _ in range(20):
                distance()
                align()
            torch.cuda.synchronize()
            assert torch.equal(dist, dist2) and torch.equal(units, units2)
            t_d, t_a = [], []
            for _ in range(windows):
                t_d.append(window(distance, reps))
                t_a.append(window(align, reps))
            rec = {"edit_distance_us": round(statistics.median(t_d), 2), "edit_align_us": round(statistics.median(t_a), 2),
                   "edit_distance_us_min_max": [round(min(t_d), 2), round(max(t_d), 2)],
                   "edit_align_us_min_max": [round(min(t_a), 2), round(max(t_a), 2)],
                   "mean_script_length": round(float(n_ops.float().mean()), 1), "mean_distance": round(float(dist.float().mean()), 1)}
            rec["ratio"] = round(rec["edit_align_us"] / rec["edit_distance_us"], 2)
            out["cases"]["%s_%s" % (kind, mode)] = rec
            print("%-9s %-6s distance %.2f us  align %.2f us  (x%.2f), script %.0f ops" % (kind, mode, rec["edit_distance_us"],
                                                                                         rec["edit_align_us"], rec["ratio"], rec["mean_script_length"]))
    out["workspace_bytes"] = nb
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "edit_ops_time.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
