"""Times of streaming recognition on one GPU -> profiles/streaming_time.md.  Recorded, not gated: these numbers did not exist
before the feature.

  1. The decoder: HIP events around a one-shot beam decode of T = 500 frames against the same frames fed to ops.CtcBeamStream in
     ten 50-frame chunks, for C = 28 and C = 4334, beam widths 16 and 128, without an LM and with a character 3-gram.  With
     --parent-lib PATH (a liblasr.so built from the parent commit) the one-shot time of that library is taken in the same call,
     in a child process that loads it through LASR_LIB_PATH.
  2. The recogniser: host time per feed() (a device synchronise after each) and the real-time factor at the default contexts,
     for the plain and the q105 variant with freshly initialised weights, greedy and beam (width 16), 0.1 s packets of a 20 s
     synthetic recording.

    python tools/streaming_time.py [--parent-lib build_parent/liblasr.so] [--out profiles/streaming_time.md]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

T, CHUNK, REPS = 500, 50, 20
EN = ["'"] + [chr(ord("a") + i) for i in range(26)]


def peaky(Tn, Cn, seed, torch):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, Tn, Cn, generator=g) * 2.0
    hot = torch.randint(0, Cn - 1, (1, Tn), generator=g)
    hot = torch.where(torch.rand(1, Tn, generator=g) < 0.6, torch.full_like(hot, Cn - 1), hot)
    x.scatter_add_(2, hot.unsqueeze(-1), torch.full((1, Tn, 1), 8.0))
    return torch.log_softmax(x, -1)


def event_ms(fn, torch, reps=REPS):
    """median over `reps` of HIP events around fn(), after two warm-up calls"""
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def decoder_cases(one_shot_only):
    import torch
    import arpa_synth as S
    from lightning_asr_amd import ops
    dev = torch.device("cuda")
    d = tempfile.mkdtemp()
    lm_path = S.write_arpa(os.path.join(d, "en3.arpa"), EN, 3, 400, seed=3)
    rows = []
    for Cn in (28, 4334):
        x = peaky(T, Cn, 1, torch).to(dev).contiguous()
        for Wd in (16, 128):
            for with_lm in (False, True):
                if with_lm and Cn != 28:
                    continue                      # the synthetic character LM is over the 27 English labels
                lm = ops.load_arpa(lm_path, EN, dev, 0.7, 1.0) if with_lm else None
                if lm is None:
                    one = lambda: ops.ctc_beam_decode(x, None, Cn - 1, Wd, 40, 1.0, 1)
                else:
                    one = lambda: ops.ctc_beam_decode_lm(x, None, Cn - 1, lm, Wd, 40, 1.0, 1)
                r = {"C": Cn, "W": Wd, "lm": with_lm, "one_shot_ms": event_ms(one, torch)}
                if not one_shot_only:
                    st = ops.CtcBeamStream(1, Cn, Cn - 1, Wd, 40, 1.0, 1, T, lm=lm, device=dev)
                    chunks = [x[:, s:s + CHUNK].contiguous() for s in range(0, T, CHUNK)]

                    def fed():
                        st.reset()
                        for c in chunks:
                            st.feed(c)
                    r["stream_ms"] = event_ms(fed, torch)
                    want = one()
                    torch.cuda.synchronize()
                    r["equal"] = bool(torch.equal(st.tokens, want[0]) and torch.equal(st.scores, want[2]))
                rows.append(r)
    return rows


def recogniser_cases():
    import torch
    from lightning_asr_amd.predict import AsrTranslator, EN_LABELS
    from lightning_asr_amd.train import LightingModule
    d = tempfile.mkdtemp()
    secs, packet = 20.0, 1600
    n = int(16000 * secs)
    t = torch.arange(n) / 16000.0
    wave = (0.3 * torch.sin(2 * math.pi * (220 + 40 * t) * t) * (0.5 + 0.5 * torch.sin(2 * math.pi * 2.0 * t))
            + 0.02 * torch.randn(n, generator=torch.Generator().manual_seed(0))).clamp(-1, 1)
    rows = []
    for variant in ("plain", "q105"):
        torch.manual_seed(0)
        model = LightingModule(labels=EN_LABELS, variant=variant)
        path = os.path.join(d, variant + ".ckpt")
        torch.save({"state_dict": model.state_dict(), "hyper_parameters": dict(labels=EN_LABELS, variant=variant, mask=True)}, path)
        del model
        for decoder in ("greedy", "beam"):
            tr = AsrTranslator(path, map_location="cuda", decoder=decoder, beam_width=16)
            rec = tr.stream()
            for rep in range(2):                  # the first recording warms every shape up
                feeds, work = [], []
                for i in range(0, n, packet):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    before = rec.frames
                    rec.feed(wave[i:i + packet])
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3
                    feeds.append(dt)
                    if rec.frames > before:
                        work.append(dt)
                t0 = time.perf_counter()
                rec.finish()
                torch.cuda.synchronize()
                fin = (time.perf_counter() - t0) * 1e3
            rows.append({"variant": variant, "decoder": decoder, "feeds": len(feeds), "feed_ms_median": sorted(feeds)[len(feeds) // 2],
                         "window_feed_ms_median": sorted(work)[len(work) // 2], "window_feed_ms_max": max(work),
                         "windows": len(work), "finish_ms": fin, "rtf": (sum(feeds) + fin) / 1e3 / secs})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streaming_time.md"))
    ap.add_argument("--one-shot-json", action="store_true", help="(child) print the one-shot times of the loaded library as JSON")
    a = ap.parse_args()
    if a.one_shot_json:
        from lightning_asr_amd import _lib
        for name in [k for k in _lib.SIGNATURES if "beam_stream" in k]:
            del _lib.SIGNATURES[name]             # the parent's library does not export them, and this process does not call them
        print("JSON " + json.dumps(decoder_cases(True)))
        return
    dec = decoder_cases(False)
    parent = None
    if a.parent_lib:
        env = dict(os.environ, LASR_LIB_PATH=os.path.abspath(a.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-shot-json"], env=env, check=True, stdout=subprocess.PIPE,
                             timeout=300).stdout.decode()
        parent = json.loads([l for l in out.splitlines() if l.startswith("JSON ")][-1][5:])
    recs = recogniser_cases()
    L = ["# Streaming recognition: measured times", "",
         "One MI355X, `tools/streaming_time.py`.  Recorded, not gated.", "",
         "## Decoder: one-shot against ten 50-frame feeds (T = 500, B = 1, cutoff_top_n 40, n_best 1)", "",
         "HIP events around the calls, median of %d after two warm-up calls; the streamed figure includes the reset and, per feed, the" % REPS,
         "prune and search launches with the load and store of the state.  `equal`: tokens and scores of the last feed against the",
         "one-shot call.  `parent`: the one-shot call of the parent commit's library, measured in a child process of the same run.", "",
         "| C | beam width | LM | one-shot ms | parent one-shot ms | ten feeds ms | streamed / one-shot | equal |", "|---|---|---|---|---|---|---|---|"]
    for i, r in enumerate(dec):
        p = "%.3f" % parent[i]["one_shot_ms"] if parent else "-"
        L.append("| %d | %d | %s | %.3f | %s | %.3f | %.2f | %s |" % (r["C"], r["W"], "character 3-gram" if r["lm"] else "none", r["one_shot_ms"],
                                                                    p, r["stream_ms"], r["stream_ms"] / r["one_shot_ms"], r["equal"]))
    L += ["", "## Recogniser: `AsrTranslator.stream()` at the defaults (chunk 1.0 s, left 4.0 s, right 1.0 s)", "",
          "A 20 s synthetic recording in 0.1 s packets, freshly initialised weights (f32), dither on, second pass over the recording;",
          "host clock with a device synchronise after every feed.  A feed that completes a step runs one window (up to 6 s of audio)",
          "through features, model and decoder; the other feeds only append samples.  Real-time factor = all feeds + finish over 20 s.", "",
          "| variant | decoder | feeds | median feed ms | windows | median window feed ms | max window feed ms | finish ms | real-time factor |",
          "|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        L.append("| %s | %s | %d | %.3f | %d | %.2f | %.2f | %.2f | %.4f |" % (r["variant"], r["decoder"], r["feeds"], r["feed_ms_median"],
                                                                          r["windows"], r["window_feed_ms_median"], r["window_feed_ms_max"],
                                                                          r["finish_ms"], r["rtf"]))
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
