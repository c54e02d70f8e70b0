"""Time lasr_ctc_beam_decode_lm (prune launch + LM-fused search launch) next to lasr_ctc_beam_decode on the same inputs, with HIP
events: cfg2 (B=32, T'=501, C=28, beam 32) and cfg5 (B=32, T'=801, C=4334, beams 32 and 64), cutoff_top_n 40, alpha 0.5,
beta 1.0.  LMs are synthetic character ARPA files (tests/helpers/arpa_synth.py): for C=28 a 3-gram and a 6-gram over the
English letters; for C=4334 a 3-gram of about 1 M n-grams and a 6-gram over an AISHELL-sized vocabulary.  Inputs are peaky
log-softmaxed normals (tools/beam_time.py).  Prints one JSON line per (shape, LM, beam); --out writes them as JSONL.

    python tools/beam_lm_time.py [--reps N] [--out profiles/r07_beam_lm_time.jsonl] [--dump FILE.npz]

--dump saves every timed case's outputs (tokens, n_tokens, scores and, with an LM, am_scores), as tools/beam_time.py does."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import torch  # noqa: E402

import arpa_synth as S  # noqa: E402
from lightning_asr_amd import ops  # noqa: E402
from tools.beam_time import dump_case, peaky, save_dump, timed  # noqa: E402

EN = ["'"] + [chr(ord("a") + i) for i in range(26)]               # data/labels.txt: C = 28 with the blank
HAN = [chr(0x4E00 + i) for i in range(4333)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp()
    t0 = time.time()
    lms = {
        "c28_3gram": (EN, S.write_arpa(os.path.join(tmp, "en3.arpa"), EN, 3, 20000, seed=1)),
        "c28_6gram": (EN, S.write_arpa(os.path.join(tmp, "en6.arpa"), EN, 6, 20000, seed=2)),
        "c4334_3gram": (HAN, S.write_arpa(os.path.join(tmp, "han3.arpa"), HAN, 3, 120000, seed=3)),
        "c4334_6gram": (HAN, S.write_arpa(os.path.join(tmp, "han6.arpa"), HAN, 6, 30000, seed=4)),
    }
    print("# LMs written in %.1f s" % (time.time() - t0), flush=True)
    shapes = [("cfg2", 32, 501, 28, (32,), ("c28_3gram", "c28_6gram")),
              ("cfg5", 32, 801, 4334, (32, 64), ("c4334_3gram", "c4334_6gram"))]
    lines, dump = [], {}
    for name, B, T, C, widths, lm_names in shapes:
        x = peaky(B, T, C, 1, dev)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        for W in widths:
            base, base_min, out = timed(lambda: ops.ctc_beam_decode(x, lens, C - 1, W, 40, 1.0, 1), a.reps)
            dump_case(dump, "%s.w%d.no_lm" % (name, W), out)
            for lm_name in lm_names:
                vocab, path = lms[lm_name]
                t1 = time.time()
                lm = ops.load_arpa(path, vocab, dev, 0.5, 1.0)
                load_s = time.time() - t1
                ms, ms_min, out = timed(lambda: ops.ctc_beam_decode_lm(x, lens, C - 1, lm, W, 40, 1.0, 1), a.reps)
                dump_case(dump, "%s.w%d.%s" % (name, W, lm_name), out, ("tokens", "n_tokens", "scores", "am_scores"))
                rec = {"shape": name, "B": B, "T": T, "C": C, "beam_width": W, "cutoff_top_n": 40, "lm": lm_name,
                       "order": lm.order, "n_ngrams": lm.n_ngrams, "image_mb": round(lm.image.numel() / 2 ** 20, 2),
                       "load_s": round(load_s, 2), "ms_median": round(ms, 3), "ms_min": round(ms_min, 3),
                       "no_lm_ms_median": round(base, 3), "no_lm_ms_min": round(base_min, 3),
                       "lm_us_per_frame": round(1000.0 * (ms - base) / T, 2), "reps": a.reps,
                       "mean_tokens": round(float(out[1].float().mean()), 1)}
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
