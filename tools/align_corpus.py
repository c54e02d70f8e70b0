"""Cut long recordings with their transcripts into a training corpus: AsrTranslator.cut_corpus over a list of pairs.

  python tools/align_corpus.py CKPT PAIRS OUT_DIR MANIFEST [--max-duration 16.7] [--min-score X] [--band 4096] [--max-band 8192]
                               [--window-s 20] [--context-s 4] [--batch-size 8] [--resample]

PAIRS: a text file, one pair per line, `<audio path><TAB><transcript path>`.  A transcript file holds the recording's text in
reading order, one sentence per line (empty lines are skipped, a line's outer whitespace is dropped; nothing else is normalised:
every character has to be in the model's vocabulary).  Utterance wavs go to OUT_DIR/<audio stem>_<first sentence>.wav, their
lines {"audio_filepath", "duration", "text", "score"} are appended to MANIFEST, the format LibriDataModule trains on.  A pair
whose alignment fails (a transcript too long for its audio, a path the band loses) is reported and skipped."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_pairs(path):
    pairs = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            if len(parts) != 2:
                raise ValueError("%s:%d: expected `<audio path><TAB><transcript path>`" % (path, n))
            pairs.append((parts[0].strip(), parts[1].strip()))
    return pairs


def read_sentences(path):
    with open(path, encoding="utf-8") as f:
        return [s for s in (line.strip() for line in f) if s]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("ckpt")
    ap.add_argument("pairs")
    ap.add_argument("out_dir")
    ap.add_argument("manifest")
    ap.add_argument("--max-duration", type=float, default=16.7)
    ap.add_argument("--min-score", type=float, default=None)
    ap.add_argument("--band", type=int, default=4096)
    ap.add_argument("--max-band", type=int, default=8192, help="the widest band to escalate to; the kernel takes at most 8192")
    ap.add_argument("--window-s", type=float, default=20.0)
    ap.add_argument("--context-s", type=float, default=4.0)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--resample", action="store_true")
    a = ap.parse_args(argv)
    from lightning_asr_amd.predict import AsrTranslator
    tr = AsrTranslator(a.ckpt, map_location="cuda", resample=a.resample)
    n_utt, secs, failed = 0, 0.0, 0
    for audio, transcript in read_pairs(a.pairs):
        try:
            res = tr.cut_corpus(audio, read_sentences(transcript), a.out_dir, a.manifest, max_duration=a.max_duration, min_score=a.min_score,
                                band=a.band, max_band=a.max_band, window_s=a.window_s, context_s=a.context_s, batch_size=a.batch_size)
        except ValueError as e:
            failed += 1
            print("%s: skipped: %s" % (audio, e))
            continue
        kept = sum(u["duration"] for u in res["utterances"])
        n_utt += len(res["utterances"])
        secs += kept
        print("%s: %.1f s, band %d, %d utterances (%.1f s), %d dropped" % (audio, res["duration"], res["band"], len(res["utterances"]), kept,
                                                                          len(res["dropped"])))
    print("%d utterances, %.2f h, %d recordings skipped -> %s" % (n_utt, secs / 3600.0, failed, a.manifest))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
