"""Dev tool: time lasr_ctc_kws next to lasr_ctc_align of the same shape in the same process: cfg2 (B=32, T'=501, C=28: emission
rows staged in LDS) and cfg5 (C=4334: row-maximum pre-pass + global gather) with K = 1, 32 and 256 phrases of 4 to 24 labels, and
B=1 with K=256 (the find_keywords case: the parallelism comes from K alone).  Events around `reps` replays after warm-up,
workspaces and outputs allocated once.  Writes profiles/ctc_kws_time.json.
python tools/kws_time.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from lightning_asr_amd import _lib, ops  # noqa: E402

SHAPES = {"cfg2": (32, 501, 28, 150), "cfg5": (32, 501, 4334, 150)}      # B, T', C, S of the alignment timed beside it
CASES = [("cfg2", 32, 1), ("cfg2", 32, 32), ("cfg2", 32, 256), ("cfg2", 1, 256), ("cfg5", 32, 1), ("cfg5", 32, 32), ("cfg5", 32, 256),
         ("cfg5", 1, 256)]
MAX_HITS = 8


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device("cuda")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = {"reps": reps, "unit": "us per call", "max_hits": MAX_HITS, "threshold": -2.0, "phrase_labels": [4, 24], "cases": []}
    align_us = {}
    for name, B, K in CASES:
        _, T, C, S = SHAPES[name]
        g = torch.Generator().manual_seed(1)
        logp = torch.randn(B, T, C, generator=g).log_softmax(-1).to(dev).contiguous()
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        if (name, B) not in align_us:                                        # lasr_ctc_align at the same B, T', C
            tg = torch.randint(0, C - 1, (B, S), generator=g).to(dev)
            tl = torch.full((B,), S, dtype=torch.int32, device=dev)
            al = ops.ctc_align(logp, tg, il, tl, C - 1)
            nb_al = int(lib.lasr_ctc_align_workspace_bytes(B, T, S))
            ws_al = torch.empty(max(nb_al, 256), dtype=torch.uint8, device=dev)

            def align():
                _lib.call("lasr_ctc_align", logp.data_ptr(), tg.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, C, S, C - 1,
                          al.score.data_ptr(), al.frame_state.data_ptr(), al.frame_logp.data_ptr(), al.label_start.data_ptr(),
                          al.label_end.data_ptr(), ws_al.data_ptr(), nb_al, st)

            align_us[(name, B)] = timed(align, reps)
        lens = torch.randint(4, 25, (K,), generator=g).tolist()
        phrases = []
        for n in lens:                                                       # labels without an adjacent repeat: every phrase fits
            p = torch.randint(0, C - 1, (n,), generator=g).tolist()
            for i in range(1, n):
                if p[i] == p[i - 1]:
                    p[i] = (p[i] + 1) % (C - 1)
            phrases.append(p)
        bank = ops.build_keywords(phrases, n_classes=C, blank=C - 1, device=dev)
        hits = ops.ctc_keyword_search(logp, il, C - 1, bank, -2.0, MAX_HITS)   # outputs reused below
        nb = int(lib.lasr_ctc_kws_workspace_bytes(B, T, K))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def kws():
            _lib.call("lasr_ctc_kws", logp.data_ptr(), il.data_ptr(), B, T, C, C - 1, bank.labels.data_ptr(), bank.offsets.data_ptr(), K,
                      bank.max_len, -2.0, MAX_HITS, hits.n_hits.data_ptr(), hits.hit_span.data_ptr(), hits.hit_score.data_ptr(),
                      hits.best_score.data_ptr(), hits.best_span.data_ptr(), ws.data_ptr(), nb, st)

        t_kws = timed(kws, reps)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(hits.best_score).all()) and bool((hits.best_score <= 0).all())
        rec = {"shape": name, "B": B, "T": T, "C": C, "K": K, "pairs": B * K, "max_labels": bank.max_len,
               "ctc_kws_us": round(t_kws, 1), "ctc_align_us_same_B_T_C": round(align_us[(name, B)], 1), "align_S": S,
               "workspace_bytes": nb, "hits_total": int(hits.n_hits.sum())}
        out["cases"].append(rec)
        print("%-4s B=%-2d T'=%d C=%-4d K=%-3d: lasr_ctc_kws %8.1f us   lasr_ctc_align (S=%d) %8.1f us" % (name, B, T, C, K, t_kws, S,
                                                                                                         align_us[(name, B)]))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ctc_kws_time.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
