"""Time lasr_ctc_beam_decode_wlm (prune launch + word-LM search launch) next to lasr_ctc_beam_decode_lm and lasr_ctc_beam_decode
on the same inputs, with HIP events, as tools/beam_lm_time.py does for the character LM: B=32, T'=501, C=29 (predict.EN_LABELS),
beam 40, cutoff_top_n 40, alpha 0.5, beta 1.0.  The word LM is a synthetic 3-gram over a 20 000-word lexicon of the English
letters (tests/helpers/wlm_synth.py, arpa_synth.py); the character LM a synthetic 3-gram over the same labels.  Inputs are
log-probs peaky around sentences of the lexicon's words, T' frames each.  Prints one JSON line; --out writes it as JSONL.

    python tools/beam_wlm_time.py [--reps N] [--words N] [--out profiles/beam_wlm_time.jsonl] [--dump FILE.npz]

--dump saves the three decodes' outputs (tokens, n_tokens, scores and, with an LM, am_scores), as tools/beam_time.py does.

The three decodes alternate inside each of --rounds rounds, so that a drift of the clock falls on all of them alike."""
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
import wlm_synth as WS  # noqa: E402
from lightning_asr_amd import ops  # noqa: E402
from lightning_asr_amd.predict import EN_LABELS  # noqa: E402
from tools.beam_time import dump_case, save_dump, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    tmp = tempfile.mkdtemp()
    B, T, W, K = 32, 501, 40, 40
    C = len(EN_LABELS) + 1
    t0 = time.time()
    words = WS.random_words(a.words, EN_LABELS[1:], 7, 1, 9)
    sents = [words[i:i + 10] for i in range(0, len(words), 10)] + S.sentences(words, 20000, 1)
    wpath = os.path.join(tmp, "words3.arpa")
    with open(wpath, "w", encoding="utf-8") as f:
        f.write(S.arpa_text(sents, 3))
    cpath = S.write_arpa(os.path.join(tmp, "chars3.arpa"), EN_LABELS, 3, 20000, seed=1)
    print("# LMs written in %.1f s" % (time.time() - t0), flush=True)
    t1 = time.time()
    wlm = ops.load_arpa(wpath, EN_LABELS, dev, 0.5, 1.0)
    load_s = time.time() - t1
    clm = ops.load_arpa(cpath, EN_LABELS, dev, 0.5, 1.0)
    assert not wlm.is_character_based() and clm.is_character_based()
    x, _ = WS.sentence_logp(EN_LABELS, words, B, T, 1, hot=10.0, n_words=(60, 80))
    x = x.to(dev).contiguous()
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    fns = {"word_lm": lambda: ops.ctc_beam_decode_lm(x, lens, C - 1, wlm, W, K, 1.0, 1),
           "char_lm": lambda: ops.ctc_beam_decode_lm(x, lens, C - 1, clm, W, K, 1.0, 1),
           "no_lm": lambda: ops.ctc_beam_decode(x, lens, C - 1, W, K, 1.0, 1)}
    ms, mins = {k: [] for k in fns}, {k: [] for k in fns}
    outs = {}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            med, mn, outs[k] = timed(fn, a.reps)
            ms[k].append(med)
            mins[k].append(mn)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    rec = {"B": B, "T": T, "C": C, "beam_width": W, "cutoff_top_n": K, "order": wlm.order, "n_lexicon_words": wlm.n_lexicon_words,
           "word_n_ngrams": wlm.n_ngrams, "word_image_mb": round(wlm.image.numel() / 2 ** 20, 2), "word_load_s": round(load_s, 2),
           "char_n_ngrams": clm.n_ngrams, "char_image_mb": round(clm.image.numel() / 2 ** 20, 2),
           "word_lm_ms": round(med["word_lm"], 3), "char_lm_ms": round(med["char_lm"], 3), "no_lm_ms": round(med["no_lm"], 3),
           "word_over_char": round(med["word_lm"] / med["char_lm"], 3), "rounds_ms": {k: [round(v, 3) for v in vs] for k, vs in ms.items()},
           "ms_min": {k: round(min(vs), 3) for k, vs in mins.items()},
           "reps": a.reps, "rounds": a.rounds,
           "mean_tokens": {k: round(float(o[1].float().mean()), 1) for k, o in outs.items()}}
    print(json.dumps(rec), flush=True)
    if a.dump:
        dump = {}
        for k, o in outs.items():
            dump_case(dump, k, o, ("tokens", "n_tokens", "scores", "am_scores"))
        save_dump(a.dump, dump)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
