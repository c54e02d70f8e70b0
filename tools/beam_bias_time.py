"""Time the hotword-biased beam search (ops.ctc_beam_decode_biased: prune launch + biased search launch) next to the unbiased
search on the same inputs, inside one process, with HIP events: B = 32, T' = 501 at (C = 28, beams 16 and 128) and (C = 4334,
beam 16), cutoff_top_n 40, banks of 0, 1, 100 and 10 000 random phrases of 2..6 labels (weight 2.0; the single phrase has 6
labels: the larger banks' max_credit, so their slack in the LM search's early cutoff, with next to no walks).  The reference is
ops.ctc_beam_decode of a second build of the library when --parent names one (the parent commit's liblasr.so, loaded beside
this build's), else this build's.  With --lm the character-LM variant is timed against ops.ctc_beam_decode_lm too (a synthetic
3-gram, tests/helpers/arpa_synth.py).  Calls are interleaved round by round (reference, then each bank), so that clock drift
falls on all of them alike; inputs are peaky log-softmaxed normals (tools/beam_time.py).  One JSON line per case.

    python tools/beam_bias_time.py [--reps N] [--parent PATH/liblasr.so] [--lm] [--out profiles/beam_bias_time.jsonl] [--dump F.npz]

--dump saves every timed case's outputs (tokens, n_tokens, scores and, where the search has them, am_scores and bias_scores),
as tools/beam_time.py does."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import arpa_synth as S  # noqa: E402
from lightning_asr_amd import _lib, ops  # noqa: E402
from tools.beam_time import dump_case, peaky, save_dump  # noqa: E402

EN = ["'"] + [chr(ord("a") + i) for i in range(26)]
HAN = [chr(0x4E00 + i) for i in range(4333)]


def parent_decode(path):
    """ops.ctc_beam_decode through another build of the library (same arguments, same workspace rule)"""
    lib = ctypes.CDLL(path)
    res, args = _lib.SIGNATURES["lasr_ctc_beam_decode"]
    lib.lasr_ctc_beam_decode.restype, lib.lasr_ctc_beam_decode.argtypes = res, args
    lib.lasr_ctc_beam_workspace_bytes.restype, lib.lasr_ctc_beam_workspace_bytes.argtypes = _lib.SIGNATURES["lasr_ctc_beam_workspace_bytes"]

    def decode(x, lens, blank, W, k, cp, n_best):
        B, T, C = x.shape
        nb = int(lib.lasr_ctc_beam_workspace_bytes(B, T, C, W, min(k, C)))
        tok = torch.empty(B, n_best, T, dtype=torch.int32, device=x.device)
        n = torch.empty(B, n_best, dtype=torch.int32, device=x.device)
        sc = torch.empty(B, n_best, dtype=torch.float32, device=x.device)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        rc = lib.lasr_ctc_beam_decode(x.data_ptr(), lens.data_ptr(), B, T, C, blank, W, min(k, C), cp, n_best, tok.data_ptr(),
                                      n.data_ptr(), sc.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        return tok, n, sc
    return decode


def interleaved(fns, reps):
    """{name: (median ms, min ms)} of each fn over `reps` rounds of HIP-event timings, one call of each per round, after two
    warm-up rounds"""
    for _ in range(2):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(min(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--lm", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    ref = parent_decode(a.parent) if a.parent else ops.ctc_beam_decode
    tmp = tempfile.mkdtemp()
    lines, dump = [], {}
    for name, C, widths, vocab in (("c28", 28, (16, 128), EN), ("c4334", 4334, (16,), HAN)):
        B, T = 32, 501
        x = peaky(B, T, C, 1, dev)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(7)
        winners = [int(c) for c in x.argmax(-1).flatten().tolist() if c != C - 1]
        banks = {}
        for n in (0, 1, 100, 10000):
            # phrases over the labels the frames favour, so that the automaton is walked, not only probed at the root.  The bank
            # of one phrase has six labels: the max_credit of the larger banks (12), so the same slack in the LM search's early
            # cutoff, and next to no walks
            phrases = [[winners[int(i)] for i in rng.integers(0, len(winners), 6 if n == 1 else int(rng.integers(2, 7)))] for _ in range(n)]
            banks[n] = ops.build_hotwords(phrases, 2.0, n_classes=C, blank=C - 1, device=dev)
        lm = ops.load_arpa(S.write_arpa(os.path.join(tmp, name + ".arpa"), vocab, 3, 20000, seed=1), vocab, dev, 0.5, 1.0) if a.lm else None
        for W in widths:
            fns = {"reference": lambda: ref(x, lens, C - 1, W, 40, 1.0, 1), "unbiased": lambda: ops.ctc_beam_decode(x, lens, C - 1, W, 40, 1.0, 1)}
            for n, bank in banks.items():
                fns["bias_%d" % n] = lambda bank=bank: ops.ctc_beam_decode_biased(x, lens, C - 1, bank, W, 40, 1.0, 1)
            if lm is not None:
                fns["lm"] = lambda: ops.ctc_beam_decode_lm(x, lens, C - 1, lm, W, 40, 1.0, 1)
                for n, bank in banks.items():
                    fns["lm_bias_%d" % n] = lambda bank=bank: ops.ctc_beam_decode_biased(x, lens, C - 1, bank, W, 40, 1.0, 1, lm)
            t = interleaved(fns, a.reps)
            if a.dump:
                for k, f in fns.items():
                    dump_case(dump, "%s.w%d.%s" % (name, W, k), f(), ("tokens", "n_tokens", "scores", "am_scores", "bias_scores"))
            out0 = ops.ctc_beam_decode_biased(x, lens, C - 1, banks[0], W, 40, 1.0, 1)
            same = all(torch.equal(u, v) for u, v in zip(out0[:3], ref(x, lens, C - 1, W, 40, 1.0, 1)))
            rec = {"shape": name, "B": B, "T": T, "C": C, "beam_width": W, "cutoff_top_n": 40, "reps": a.reps,
                   "reference": "parent build" if a.parent else "this build", "empty_bank_equals_reference": bool(same),
                   "bank_nodes": {str(n): b.n_nodes for n, b in banks.items()},
                   "bank_image_kb": {str(n): round(b.image.numel() / 1024, 1) for n, b in banks.items()},
                   "ms_median": {k: round(v[0], 3) for k, v in t.items()}, "ms_min": {k: round(v[1], 3) for k, v in t.items()}}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.dump:
        save_dump(a.dump, dump)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
