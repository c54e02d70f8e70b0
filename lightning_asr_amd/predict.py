"""Inference surface of the reference (predict.py:21-74): checkpoint -> ``AsrTranslator.translate`` and
manifest evaluation, on the HIP path (mel front-end, eval-mode model forward, greedy CTC decode - or, with
``decoder="beam"``, the CTC prefix beam search of beam_search.py, fused with an n-gram LM when ``lm_path`` names a text ARPA
file: a character LM, or - the labels having exactly one " ", as EN_LABELS has - a word LM with its lexicon).
``error_report`` splits a manifest's WER / CER into substitutions, deletions and insertions (``ops.edit_ops_batch``: the aligned reference and hypothesis of every utterance, the most confused pairs).
``translate_long`` takes a recording of any length: cut into utterances on the device (``ops.vad_segments``), decoded in batches, times relative to the recording.
``align`` / ``translate_timed`` / ``align_manifest`` add word timings: the CTC forced alignment of a known transcript (or of the decoder's own hypothesis) to the audio, ``ops.ctc_align`` + the record functions of align.py.
``encode_long`` / ``align_long`` / ``cut_corpus`` go the other way at scale: the log-probs of a whole recording (overlapping windows, batched), the banded forced alignment of its transcript (``ops.ctc_align_long``), and utterance wavs + a training manifest cut from it.
``find_keywords`` / ``find_keywords_long`` / ``keyword_scores`` spot phrases in the frame posteriors with time spans and scores, without decoding: ``ops.ctc_keyword_search`` + the record functions of kws.py.

The checkpoint is the PL-style dict the reference's ``ModelCheckpoint`` writes and ``Trainer`` here
writes too: ``state_dict`` with the reference's key names (``encoder.encoder.block1.seq.0...``) and
``hyper_parameters`` (train.py:194 ``save_hyperparameters``), so reference-trained weights load as-is.
The SSL / LM-beam-search translator (predict.py:76-) belongs to the wav2vec2 branch, out of scope."""
from __future__ import annotations

import json
import math
import os
import time
from collections import Counter
from typing import List, Optional, Tuple

import torch

from .align import frame_seconds, unit_records
from .kws import hit_records, score_records, sort_records
from .data_module import AudioParser, LibriDataModule, load_wav, load_wav_rate
from .lightning_compat import Trainer
from .train import LightingModule
from . import ops
from .beam_search import BeamSearchDecoderWithLM
from .utils.asr_metrics import WER, _alignment, _edit_ops, word_error_rate

EN_LABELS = [" ", "'"] + [chr(ord("a") + i) for i in range(26)]
# the narrowest batch the model's forward takes is 33 feature frames (lasr_model_forward): 1 + (L + 64) // 160 >= 33.  A batch of
# short segments is gathered into rows at least this wide; each row keeps its own length.
MIN_ROW_SAMPLES = 160 * (33 - 1) - 64


class AsrTranslator:
    def __init__(self, model_path: str, map_location: str = "cuda", lang: str = "en", labels: Optional[List[str]] = None,
                 verbose: bool = False, decoder: str = "greedy", beam_width: int = 16, cutoff_top_n: int = 40,
                 cutoff_prob: float = 1.0, lm_path: Optional[str] = None, alpha: float = 1.0, beta: float = 1.0, resample: bool = False,
                 hotwords=None, hotword_weight: float = 2.0, use_ema: Optional[bool] = None):
        """model_path: a ``.ckpt`` written by the reference or by ``Trainer``; map_location must name a GPU
        ("cuda" / "cuda:0"): there is no CPU path.  ``labels`` overrides the language's vocabulary.
        decoder: "greedy" (argmax + CTC collapse, the default) or "beam" (CTC prefix beam search; with ``lm_path``, a text ARPA
        LM, fused with it: ``alpha`` weighs the LM, ``beta`` is the per-label bonus of a character LM and the per-word bonus
        of a word LM, under which only the LM's words are decoded).
        hotwords: a list of ``str`` or ``(str, weight)`` the beam search is biased towards (names, product terms, contacts),
        with or without a character LM; every beam path picks them up (``translate``, ``translate_nbest``, ``translate_timed``,
        ``translate_long``, ``evalute_manifest`` and ``error_report`` with decoder="beam").  ``hotword_weight`` is the weight of a
        phrase given without one, in natural-log units per matched label; the default 2.0 is a starting value: nobody has tuned
        it on a trained model.  decoder="greedy" with hotwords raises ValueError, a word-level LM NotImplementedError;
        ``set_hotwords`` swaps the bank later.
        use_ema: which weights of a checkpoint whose run kept a weight EMA (``train.ema_decay`` > 0): None (the default) - the
        averaged ones when the checkpoint has them, the live ones otherwise, so every other checkpoint loads as it always did;
        True - the averaged ones, ValueError when the checkpoint has none; False - the live ones.
        resample: False (the default, the reference's behaviour) feeds a file's samples to the 16 kHz front-end whatever its
        sample rate; True converts a file of another rate on the device first (``ops.resample``) - ``translate``,
        ``translate_nbest``, ``align`` and ``translate_timed`` then hear it at its true speed and report its true times (each
        takes ``resample=`` to override the translator's setting for one call); ``evalute_manifest`` / ``align_manifest`` do not
        resample: with resample=True they refuse a manifest that holds a file of another rate."""
        if decoder not in ("greedy", "beam"):
            raise ValueError("decoder must be 'greedy' or 'beam', got %r" % (decoder,))
        if hotwords and decoder != "beam":
            raise ValueError("hotwords bias the beam search: decoder must be 'beam', got %r" % (decoder,))
        if labels is not None:
            self.labels = list(labels)
        elif lang == "en":
            self.labels = list(EN_LABELS)
        else:
            raise Exception("其他语言未实现")                      # predict.py:36
        if not str(map_location).startswith("cuda"):
            raise ValueError("AsrTranslator runs on the GPU only (map_location=%r)" % (map_location,))
        self.model_path = model_path
        self.map_location = map_location
        self.verbose = verbose
        self.model = LightingModule.load_from_checkpoint(model_path, map_location=map_location, use_ema=use_ema, device=str(map_location))
        self.audio_parser = AudioParser(device=str(map_location))
        self.audio_parser.act_dtype = self.model.encoder.native.act_dtype
        self.device = torch.device(map_location)
        self.wer = WER(vocabulary=self.labels)
        self.decoder = decoder
        self.resample = bool(resample)
        self.beam = BeamSearchDecoderWithLM(self.labels, beam_width, alpha, beta, lm_path, 1, cutoff_prob=cutoff_prob,
                                            cutoff_top_n=cutoff_top_n, device=str(map_location), hotwords=hotwords,
                                            hotword_weight=hotword_weight)
        self.model.eval()

    def set_hotwords(self, hotwords, weight: Optional[float] = None) -> None:
        """Swap the phrases the beam search is biased towards (``None`` or ``[]``: none); see ``__init__``"""
        if hotwords and self.decoder != "beam":
            raise ValueError("hotwords bias the beam search: the translator's decoder is %r" % (self.decoder,))
        self.beam.set_hotwords(hotwords, weight)

    @torch.no_grad()
    def translate(self, audio_path, resample: Optional[bool] = None) -> str:
        """One local audio file (path or file object) -> text (predict.py:44-63): no dither-free shortcut, the same
        feature chain as training without augmentation, eval-mode BN, argmax, CTC collapse."""
        t0 = time.time()
        inputs = self.audio_parser.parse_audio(audio_path, mask=False, resample=self._resample(resample))
        pct = torch.ones(inputs.shape[0], dtype=torch.float32, device=self.device)   # torch.FloatTensor([1.])  (:55)
        t1 = time.time()
        out = self.model._encode(inputs, pct)
        if self.decoder == "beam":
            t2 = time.time()
            text = self.beam(out, None)[0]
        else:
            ids = torch.argmax(out, dim=-1, keepdim=False)
            t2 = time.time()
            text = self.wer.ctc_decoder_predictions_tensor(ids)[0]
        if self.verbose:
            print("加载音频用时: %.4f  模型计算用时: %.4f  解码用时: %.4f" % (t1 - t0, t2 - t1, time.time() - t2))
        return text

    @torch.no_grad()
    def translate_nbest(self, audio_path, n: int = 5, resample: Optional[bool] = None) -> List[Tuple[str, float]]:
        """One audio file -> the n best beam hypotheses [(text, log-probability), ...], best first (any decoder setting)"""
        inputs = self.audio_parser.parse_audio(audio_path, mask=False, resample=self._resample(resample))
        pct = torch.ones(inputs.shape[0], dtype=torch.float32, device=self.device)
        out = self.model._encode(inputs, pct)
        return [(text, score) for score, text in self.beam.decode_nbest(out, None, n)[0]]

    def _resample(self, override: Optional[bool]) -> bool:
        return self.resample if override is None else bool(override)

    def _require_16k(self, manifest: str, who: str) -> None:
        """resample=True: the manifest loaders do not resample, so a file of another rate is refused by name instead of being
        decoded at the wrong speed"""
        from .ingest import wav_info
        from . import _lib
        with open(manifest, encoding="utf-8") as f:
            for line in f:
                if not line.strip():
                    continue
                path = json.loads(line)["audio_filepath"]
                try:
                    rate = wav_info(path)[2]
                except _lib.LasrError:                          # not a RIFF/WAVE file the native reader takes: whatever load_wav decodes
                    rate = load_wav_rate(path)[1]
                if rate != self.audio_parser.sr:
                    raise ValueError("%s: %s has a sample rate of %d Hz, not %d: the manifest loaders do not resample (convert the "
                                     "file, or use translate / align on it)" % (who, path, rate, self.audio_parser.sr))

    def evalute_manifest(self, test_manifest: str, batch_size: int = 32, num_workers: int = 0, decoder: Optional[str] = None):
        """WER over a manifest (predict.py:65-74; the reference's spelling kept).  decoder: None = the translator's own.
        Greedy runs Trainer.test; beam runs the same eval forward and loss, decodes with the beam search and scores its
        top hypothesis.  Both return one record per batch: test_loss, input, test_wer, pred, true, path."""
        decoder = self.decoder if decoder is None else decoder
        if decoder not in ("greedy", "beam"):
            raise ValueError("decoder must be 'greedy' or 'beam', got %r" % (decoder,))
        if self.resample:
            self._require_16k(test_manifest, "evalute_manifest")
        data_module = LibriDataModule(train_manifest=test_manifest, dev_manifest=test_manifest, test_manifest=test_manifest,
                                      dev_bs=batch_size, num_worker=num_workers, labels=self.labels,
                                      device=str(self.model.encoder.native.device), act_dtype=self.model.encoder.native.act_dtype)
        trainer = Trainer(gpus=1, device=str(self.model.encoder.native.device))
        if decoder == "greedy":
            return trainer.test(self.model, datamodule=data_module)
        return self._evaluate_beam(trainer, data_module)

    @torch.no_grad()
    def _evaluate_beam(self, trainer, dm):
        model = self.model
        model.trainer = trainer
        model.eval()
        dm.trainer = trainer
        dm.setup("test")
        loader = dm.test_dataloader()
        wer = model.wer
        outs = []
        for batch in trainer._eval_batches(loader, dm, len(loader)):
            out, loss, t_lengths, trans, trans_lengths = model._shared(batch)
            tokens, n, _ = self.beam.search(out, t_lengths, 1)
            top, n_top = tokens[:, 0, :].contiguous(), n[:, 0].clamp(min=0).contiguous()
            t_np, n_np = top.cpu().numpy(), n_top.cpu().numpy()
            pred = ["".join(self.labels[int(c)] for c in t_np[b, :n_np[b]]) for b in range(t_np.shape[0])]
            true = wer.decode_reference(trans, trans_lengths)
            if wer.device_path(top, trans):
                dist, units = ops.edit_distance_batch(top, n_top, trans.to(top.device, torch.int64).contiguous(),
                                                      trans_lengths.to(top.device, torch.int32).contiguous(), wer.space_id)
                batch_wer = dist.sum().float() / units.sum().float()
            else:
                batch_wer = torch.tensor(word_error_rate(pred, true, use_cer=wer.use_cer))
            outs.append({"test_loss": loss, "input": batch[0], "test_wer": batch_wer, "pred": pred, "true": true,
                         "path": batch[-1]})
        model.test_epoch_end(outs)
        return outs

    # ------------------------------------------------------------------------------------------ error breakdown
    @torch.no_grad()
    def error_report(self, manifest: str, out_path: str, batch_size: int = 32, decoder: Optional[str] = None, top: int = 20) -> dict:
        """evalute_manifest's loop with the alignment behind every distance (``ops.edit_ops_batch``: the canonical script of
        include/lasr.h - diagonal before deletion before insertion).  Units are the model metric's: words, or characters for a
        ``use_cer`` checkpoint.  Writes one JSON line per utterance to out_path - audio_filepath, ref, hyp, dist, hits, subs,
        dels, ins, alignment = [[ref unit or null, hyp unit or null, op], ...] with op 0 hit / 1 substitution / 2 deletion /
        3 insertion - and returns the summary: utterances, use_cer, dist, ref_units, hits, subs, dels, ins, wer, sub_rate,
        del_rate, ins_rate, top_substitutions [[ref, hyp, count], ...], top_deletions [[ref, count], ...], top_insertions
        [[hyp, count], ...] (the ``top`` most frequent of each).  The totals are accumulated on the device and read once; over
        characters the confusion counts come from the device matrix, over words (hashes on the device) from the scripts."""
        decoder = self.decoder if decoder is None else decoder
        if decoder not in ("greedy", "beam"):
            raise ValueError("decoder must be 'greedy' or 'beam', got %r" % (decoder,))
        if self.resample:
            self._require_16k(manifest, "error_report")
        model = self.model
        dev = model.encoder.native.device
        dm = LibriDataModule(train_manifest=manifest, dev_manifest=manifest, test_manifest=manifest, dev_bs=batch_size, num_worker=0,
                             labels=self.labels, device=str(dev), act_dtype=model.encoder.native.act_dtype)
        trainer = Trainer(gpus=1, device=str(dev))
        model.trainer = trainer
        model.eval()
        dm.trainer = trainer
        dm.setup("test")
        loader = dm.test_dataloader()
        wer = model.wer
        n_cls = len(self.labels)
        totals = torch.zeros(6, dtype=torch.int64, device=dev)
        confusion = torch.zeros(n_cls + 1, n_cls + 1, dtype=torch.int32, device=dev) if wer.use_cer and wer.device_ok else None
        host_totals = [0] * 6
        pairs = {1: Counter(), 2: Counter(), 3: Counter()}          # op -> Counter of (ref unit, hyp unit), from the scripts
        records = []
        for batch in trainer._eval_batches(loader, dm, len(loader)):
            out, _, t_lengths, trans, trans_lengths = model._shared(batch)
            if decoder == "beam":
                tokens, n, _ = self.beam.search(out, t_lengths, 1)
                tokens, n = tokens[:, 0, :].contiguous(), n[:, 0].clamp(min=0).contiguous()
            else:
                tokens, n = ops.greedy_decode(model.encoder.last_argmax.to(torch.int32).contiguous(), t_lengths.contiguous(), wer.blank_id)
            t_np, n_np = tokens.cpu().numpy(), n.cpu().numpy()
            hyps = ["".join(self.labels[int(c)] for c in t_np[b, :n_np[b]]) for b in range(t_np.shape[0])]
            refs = wer.decode_reference(trans, trans_lengths)
            scripts = None
            if wer.device_path(tokens, trans):
                res = ops.edit_ops_batch(tokens, n, trans.to(dev, torch.int64).contiguous(), trans_lengths.to(dev, torch.int32).contiguous(),
                                         wer.space_id, totals, confusion)
                script_np, len_np = res.ops.cpu().numpy(), res.n_ops.cpu().numpy()
                scripts = [script_np[b, :len_np[b]].tolist() for b in range(len(hyps))]
            for b, path in enumerate(batch[-1]):
                h_units, r_units = (list(hyps[b]), list(refs[b])) if wer.use_cer else (hyps[b].split(), refs[b].split())
                if scripts is None:
                    script = _edit_ops(h_units, r_units)
                    cnt = [script.count(k) for k in range(4)]
                    for k, v in enumerate([cnt[1] + cnt[2] + cnt[3], len(r_units)] + cnt):
                        host_totals[k] += v
                else:
                    script = scripts[b]
                alignment = _alignment(h_units, r_units, script)
                if confusion is None or scripts is None:
                    for r_u, h_u, op in alignment:
                        if op:
                            pairs[op][(r_u, h_u)] += 1
                cnt = [script.count(k) for k in range(4)]
                records.append({"audio_filepath": path, "ref": refs[b], "hyp": hyps[b], "dist": cnt[1] + cnt[2] + cnt[3], "hits": cnt[0],
                                "subs": cnt[1], "dels": cnt[2], "ins": cnt[3], "alignment": alignment})
        with open(out_path, "w", encoding="utf-8") as f:
            for rec in records:
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
        if confusion is not None:                                    # one read of the device matrix: its non-zero cells
            idx = confusion.nonzero().tolist()
            for (r_i, h_i), v in zip(idx, confusion[confusion != 0].tolist()):
                if r_i != h_i:
                    op = 3 if r_i == n_cls else 2 if h_i == n_cls else 1
                    pairs[op][(None if r_i == n_cls else self.labels[r_i], None if h_i == n_cls else self.labels[h_i])] += v
        dist, units, hits, subs, dels, ins = [a + b for a, b in zip(totals.tolist(), host_totals)]

        def ranked(op):
            return sorted(pairs[op].items(), key=lambda kv: (-kv[1], str(kv[0][0]), str(kv[0][1])))[:max(int(top), 0)]

        rate = (lambda v: v / units) if units else (lambda v: float("inf") if v else float("nan"))
        return {"utterances": len(records), "use_cer": bool(wer.use_cer), "dist": dist, "ref_units": units, "hits": hits, "subs": subs,
                "dels": dels, "ins": ins, "wer": rate(dist), "sub_rate": rate(subs), "del_rate": rate(dels), "ins_rate": rate(ins),
                "top_substitutions": [[r_u, h_u, v] for (r_u, h_u), v in ranked(1)],
                "top_deletions": [[r_u, v] for (r_u, _), v in ranked(2)],
                "top_insertions": [[h_u, v] for (_, h_u), v in ranked(3)]}

    # ------------------------------------------------------------------------------------------ forced alignment
    def frame_seconds(self) -> float:
        """seconds per output frame: the parser's hop times the model's time stride over the sample rate (0.02 s for the shipped
        variants: 160 samples at 16 kHz, stride 2).  The stride is read off the native model's own frame count."""
        native = self.model.encoder.native
        n = 4096
        stride = max(1, round(n / max(1, native.out_frames(2 * n) - native.out_frames(n))))
        return frame_seconds(self.audio_parser.hop_length, self.audio_parser.sr, stride)

    def text_to_ids(self, text: str) -> List[int]:
        """the dataset's char2index mapping (data_module.py MyAudioDataset); a character outside the vocabulary is an error"""
        char2index = dict((c, i) for i, c in enumerate(self.labels))
        ids = []
        for ch in text:
            if ch not in char2index:
                raise ValueError("align: character %r of the transcript is not in the vocabulary" % (ch,))
            ids.append(char2index[ch])
        return ids

    def _encode_file(self, audio_path, resample: Optional[bool] = None):
        """one audio file -> (log-probs (1, T', C) f32, duration in seconds): translate()'s feature chain and forward.  With
        resample on, the duration is the file's own: its samples over its sample rate; off, the samples are taken for 16 kHz."""
        if isinstance(audio_path, str) and not os.path.exists(audio_path):
            raise Exception("音频路径不存在 " + audio_path)
        if self._resample(resample):
            y, rate = load_wav_rate(audio_path)
            duration = y.shape[1] / float(rate)
            y = self.audio_parser.resample_to_sr(y, rate)
        else:
            y = load_wav(audio_path)
            duration = y.shape[1] / float(self.audio_parser.sr)
        inputs = self.audio_parser.features_one(y)[0]
        pct = torch.ones(inputs.shape[0], dtype=torch.float32, device=self.device)
        out = self.model._encode(inputs, pct)
        return out, duration

    def _decode(self, out) -> str:
        if self.decoder == "beam":
            return self.beam(out, None)[0]
        return self.wer.ctc_decoder_predictions_tensor(torch.argmax(out, dim=-1, keepdim=False))[0]

    def _align_ids(self, out, ids: List[int], duration: float) -> List[dict]:
        """word records of the label ids on the log-probs (1, T', C) of one utterance"""
        if not ids:
            return []
        logp = out.float().contiguous()
        tg = torch.tensor([ids], dtype=torch.int64, device=logp.device)
        tl = torch.tensor([len(ids)], dtype=torch.int32, device=logp.device)
        al = ops.ctc_align(logp, tg, None, tl, logp.shape[-1] - 1)
        if not math.isfinite(float(al.score[0])):
            raise ValueError("align: no alignment exists: the transcript (%d labels) is too long for the clip (%d frames)"
                             % (len(ids), logp.shape[1]))
        return unit_records(ids, al.label_start[0].tolist(), al.label_end[0].tolist(), al.frame_logp[0].tolist(), self.labels,
                            self.frame_seconds(), duration)

    @torch.no_grad()
    def align(self, audio_path, text: str, resample: Optional[bool] = None) -> List[dict]:
        """Forced alignment of a known transcript to one audio file: one record per word (per label for a vocabulary without a
        space), {"word", "start", "end", "score", "labels": [{"label", "start", "end", "score"}, ...]}, times in seconds.
        ValueError for a character outside the vocabulary and for a transcript too long for the clip."""
        ids = self.text_to_ids(text)
        out, duration = self._encode_file(audio_path, resample)
        return self._align_ids(out, ids, duration)

    @torch.no_grad()
    def translate_timed(self, audio_path, resample: Optional[bool] = None) -> Tuple[str, List[dict]]:
        """translate() with timings: decodes with the translator's own decoder and aligns that hypothesis on the same log-probs.
        Returns (text, word records); an empty hypothesis gives ("", [])."""
        out, duration = self._encode_file(audio_path, resample)
        text = self._decode(out)
        if not text:
            return "", []
        return text, self._align_ids(out, self.text_to_ids(text), duration)

    # ------------------------------------------------------------------------------------------ pseudo labels, confidences
    @torch.no_grad()
    def pseudo_label_manifest(self, manifest: str, out_path: str, threshold: float = 0.01, measure: str = "ref", batch_size: int = 32,
                              min_tokens: int = 1) -> dict:
        """Label an unlabelled manifest (JSON lines with audio_filepath and duration; a "text" is ignored) with the greedy
        hypotheses that are confident enough (``pseudo_label.label_loader``: measure <= threshold, at least min_tokens tokens) and
        write them to out_path as a training-format manifest with an extra "confidence" key.  Returns {"pseudo_seen",
        "pseudo_count", "pseudo_fraction"}.  The default threshold is the reference's constant; nobody has tuned it here."""
        from .pseudo_label import PseudoLabelConfig, label_loader
        if self.resample:
            self._require_16k(manifest, "pseudo_label_manifest")
        cfg = PseudoLabelConfig(manifest=manifest, start_epoch=0, every_n_epochs=1, threshold=threshold, measure=measure,
                                min_tokens=min_tokens, batch_size=batch_size)
        model = self.model
        dev = model.encoder.native.device
        dm = LibriDataModule(train_manifest=manifest, dev_manifest=manifest, test_manifest=manifest, dev_bs=batch_size, num_worker=0,
                             labels=self.labels, device=str(dev), act_dtype=model.encoder.native.act_dtype, pesudo_manifest=manifest)
        trainer = Trainer(gpus=1, device=str(dev))
        model.trainer = trainer
        dm.trainer = trainer
        dm.setup("test")
        selected, stats = label_loader(model, trainer, dm, dm.pseudo_train_dataloader(), cfg)
        with open(out_path, "w", encoding="utf-8") as f:
            for rec in selected:
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
        return stats

    @torch.no_grad()
    def utterance_confidence(self, audio_path, resample: Optional[bool] = None) -> dict:
        """The greedy hypothesis of one audio file with its confidences (``ops.greedy_confidence``): {"text", "ref", "nonblank",
        "posterior" (the three utterance measures of pseudo_label.PseudoLabelConfig; smaller = more confident), "tokens":
        [{"label", "start", "end" (seconds), "mean", "min" (of the frame maxima over the token's run, log-probs)}, ...]}."""
        out, duration = self._encode_file(audio_path, resample)
        logp = out.float().contiguous()
        blank = len(self.labels)
        gc = ops.greedy_confidence(logp, None, blank)
        post = ops.hyp_neg_logprob(logp, None, gc.tokens, gc.n_tokens, blank)
        n = int(gc.n_tokens[0])
        secs = self.frame_seconds()
        ids, st, en = gc.tokens[0, :n].tolist(), gc.tok_start[0, :n].tolist(), gc.tok_end[0, :n].tolist()
        mean, mn = gc.tok_mean[0, :n].tolist(), gc.tok_min[0, :n].tolist()
        conf = gc.conf[0].tolist()
        return {"text": "".join(self.labels[int(c)] for c in ids), "ref": float(conf[0]), "nonblank": float(conf[1]),
                "posterior": float(post[0]),
                "tokens": [{"label": self.labels[int(c)], "start": min(s * secs, duration), "end": min(e * secs, duration),
                            "mean": float(a), "min": float(b)} for c, s, e, a, b in zip(ids, st, en, mean, mn)]}

    # ------------------------------------------------------------------------------------------ long recordings
    def _segment_batch(self, wave: torch.Tensor, segs):
        """segments [(start, end), ...] in samples of the (L,) device wave -> (log-probs (n, T', C), frames (n,) int32): one gather
        into rows as wide as the longest of them (and no narrower than the model's shortest input), translate()'s feature chain on each row's own samples, the eval forward"""
        width = max(max(int(e) - int(s) for s, e in segs), MIN_ROW_SAMPLES)
        rows, lens = ops.gather_segments(wave, [(0, int(s), int(e)) for s, e in segs], width)
        inputs, pct = self.audio_parser.features_device(rows, lens, None, True, logical_len=rows.shape[1])
        out = self.model._encode(inputs, pct)
        return out, ops.mask_lengths(pct.to(out.device, torch.float32).contiguous(), out.size(1))

    def _decode_batch(self, out, t_lens) -> List[List[int]]:
        """the translator's own decoder over a batch: label ids of every row's hypothesis"""
        if self.decoder == "beam":
            tokens, n, _ = self.beam.search(out, t_lens, 1)
            tokens, n = tokens[:, 0, :], n[:, 0].clamp(min=0)
        else:
            tokens, n = ops.greedy_decode(self.model.encoder.last_argmax.to(torch.int32).contiguous(), t_lens.contiguous(), len(self.labels))
        t_h, n_h = tokens.tolist(), n.tolist()
        return [[int(c) for c in t_h[b][:n_h[b]]] for b in range(len(n_h))]

    def _align_batch(self, out, t_lens, ids: List[List[int]], segs) -> List[Optional[List[dict]]]:
        """one ops.ctc_align over a batch of segments: row b's label ids on its log-probs -> its word records with the times of the
        RECORDING: offset by the segment's start, clipped to its end.  [] for a row without labels, None for one without an
        alignment (a transcript too long for its segment)."""
        S = max([len(i) for i in ids] + [0])
        if S == 0:
            return [[] for _ in ids]
        logp = out.float().contiguous()
        tg = torch.zeros(len(ids), S, dtype=torch.int64)
        for b, i in enumerate(ids):
            tg[b, :len(i)] = torch.tensor(i, dtype=torch.int64)
        tl = torch.tensor([len(i) for i in ids], dtype=torch.int32)
        al = ops.ctc_align(logp, tg.to(logp.device), t_lens.contiguous(), tl.to(logp.device), logp.shape[-1] - 1)
        score, start, end, flp = al.score.tolist(), al.label_start.tolist(), al.label_end.tolist(), al.frame_logp.tolist()
        secs, sr = self.frame_seconds(), float(self.audio_parser.sr)
        recs: List[Optional[List[dict]]] = []
        for b, i in enumerate(ids):
            if not i:
                recs.append([])
                continue
            if not math.isfinite(score[b]):
                recs.append(None)
                continue
            t0, t1 = segs[b][0] / sr, segs[b][1] / sr
            words = unit_records(i, start[b], end[b], flp[b], self.labels, secs, t1 - t0)
            for w in words:
                for r in [w] + w["labels"]:
                    r["start"], r["end"] = min(r["start"] + t0, t1), min(r["end"] + t0, t1)
            recs.append(words)
        return recs

    @torch.no_grad()
    def translate_long(self, audio_path, batch_size: int = 32, timed: bool = True, resample: Optional[bool] = None, **vad) -> dict:
        """A recording of any length -> {"text", "duration", "segments": [{"start", "end", "text", "words"}, ...]} in time order,
        times in seconds of the recording.  The file is loaded once and cut into utterances on the device (``ops.vad_segments``;
        ``**vad`` are its keywords: on_db, off_db, floor_permille, min_level_db, max_floor_db, min_silence_s, min_speech_s, pad_s,
        max_segment_s, max_segments); the segments go through translate()'s chain in batches of at most ``batch_size``, longest
        first (the first batch sizes the model's workspace), each normalised over its own frames, and are decoded by the
        translator's own decoder.  timed: ``words`` = the forced alignment of each hypothesis (one ``ops.ctc_align`` per batch,
        the records of ``align``); False: None.  ``text`` joins the segments' texts with " " when the vocabulary has a space
        label, else with "".  An empty hypothesis stays a segment with "text": "" and "words": []; a recording without speech
        gives "text": "" and "segments": [].  ValueError when the recording has more than ``max_segments`` segments."""
        if isinstance(audio_path, str) and not os.path.exists(audio_path):
            raise Exception("音频路径不存在 " + audio_path)
        if int(batch_size) < 1:
            raise ValueError("translate_long: batch_size must be at least 1")
        if self._resample(resample):
            y, rate = load_wav_rate(audio_path)
            duration = y.shape[1] / float(rate)
            y = self.audio_parser.resample_to_sr(y, rate)
        else:
            y = load_wav(audio_path)
            duration = y.shape[1] / float(self.audio_parser.sr)
        result = {"text": "", "duration": duration, "segments": []}
        if y.shape[1] == 0:
            return result
        wave = y[0].to(self.device).contiguous()
        found = ops.vad_segments(wave, **vad)
        n = int(found.n_segs)                                            # the one read-back the host plans the batches from
        if n > found.segs.shape[0]:
            raise ValueError("translate_long: the recording has %d segments, more than max_segments=%d" % (n, found.segs.shape[0]))
        if n == 0:
            return result
        segs = [tuple(s) for s in found.segs[:n].tolist()]
        order = sorted(range(n), key=lambda i: segs[i][0] - segs[i][1])  # longest first; equal lengths in time order
        sr = float(self.audio_parser.sr)
        records: List[Optional[dict]] = [None] * n
        for k in range(0, n, int(batch_size)):
            idx = order[k:k + int(batch_size)]
            batch = [segs[i] for i in idx]
            out, t_lens = self._segment_batch(wave, batch)
            ids = self._decode_batch(out, t_lens)
            words = self._align_batch(out, t_lens, ids, batch) if timed else [None] * len(idx)
            for j, i in enumerate(idx):
                records[i] = {"start": segs[i][0] / sr, "end": segs[i][1] / sr, "text": "".join(self.labels[c] for c in ids[j]),
                              "words": words[j]}
        result["segments"] = records
        result["text"] = (" " if " " in self.labels else "").join(r["text"] for r in records)
        return result

    # ------------------------------------------------------------------------------------------ long recordings with a transcript
    def _load_wave(self, audio_path, resample: Optional[bool] = None):
        """one audio file -> (wave (L,) f32 on the device at the parser's rate, duration in seconds), as translate_long loads it"""
        if isinstance(audio_path, str) and not os.path.exists(audio_path):
            raise Exception("音频路径不存在 " + audio_path)
        if self._resample(resample):
            y, rate = load_wav_rate(audio_path)
            duration = y.shape[1] / float(rate)
            y = self.audio_parser.resample_to_sr(y, rate)
        else:
            y = load_wav(audio_path)
            duration = y.shape[1] / float(self.audio_parser.sr)
        return y[0].to(self.device).contiguous(), duration

    def _encode_wave_long(self, wave: torch.Tensor, window_s: float = 20.0, context_s: float = 4.0, batch_size: int = 8,
                          dither: bool = False) -> torch.Tensor:
        """encode_long on the (L,) device wave"""
        from . import streaming
        from .align import window_batches, window_frame_offsets
        sr = int(self.audio_parser.sr)
        if sr != 16000 or self.audio_parser.hop_length != streaming.HOP:
            raise ValueError("encode_long takes 16 kHz audio at hop %d" % streaming.HOP)
        native = self.model.encoder.native
        out_frames = lambda n_mel: int(native.out_frames(int(n_mel)))
        if out_frames(2 * 4096 + 1) - out_frames(4096 + 1) != 4096 // streaming.STRIDE:
            raise ValueError("encode_long is written for a model of time stride %d" % streaming.STRIDE)
        to_samples = lambda s: int(round(float(s) * sr / streaming.FRAME)) * streaming.FRAME
        chunk, ctx = to_samples(window_s), to_samples(context_s)
        if chunk <= 0 or ctx < 0:
            raise ValueError("encode_long: window_s must be at least one frame, context_s not negative")
        if int(batch_size) < 1:
            raise ValueError("encode_long: batch_size must be at least 1")
        total = int(wave.numel())
        n_classes = len(self.labels) + 1
        windows = streaming.plan_windows(total, True, chunk, ctx, ctx, 0, out_frames)
        T = streaming.total_frames(total, out_frames)
        offs = window_frame_offsets(windows, T, streaming.FRAME)
        logp = torch.empty(T, n_classes, dtype=torch.float32, device=self.device)
        for batch in window_batches(windows, batch_size):
            length = windows[batch[0]][1] - windows[batch[0]][0]
            rows = torch.zeros(len(batch), max(length, MIN_ROW_SAMPLES), dtype=torch.float32, device=self.device)
            for r, i in enumerate(batch):
                rows[r, :length] = wave[windows[i][0]:windows[i][1]]
            lens = torch.full((len(batch),), length, dtype=torch.int32, device=self.device)
            inputs, pct = self.audio_parser.features_device(rows, lens, None, dither, logical_len=rows.shape[1])
            out = self.model._encode(inputs, pct)
            for r, i in enumerate(batch):
                first, n = windows[i][2], windows[i][3]
                logp[offs[i]:offs[i] + n] = out[r, first:first + n].float()
        return logp

    @torch.no_grad()
    def encode_long(self, audio_path, window_s: float = 20.0, context_s: float = 4.0, batch_size: int = 8,
                    resample: Optional[bool] = None, dither: bool = False):
        """The log-probs of a WHOLE recording: (logp (T', C) f32 on the device, duration in seconds).  The recording is cut into the
        overlapping windows of ``streaming.plan_windows(total, True, window, context, context, 0)`` - ``window_s`` of new audio
        with ``context_s`` before and after it - each window goes through the feature chain and the eval forward exactly as a
        window of the streaming recogniser does (normalised over its own frames), and only the rows of its middle are kept: the
        kept rows tile the recording's ``streaming.total_frames`` exactly once.  Windows of equal sample length run together,
        ``batch_size`` per forward; the first and the last window have lengths of their own and a forward each.  With
        batch_size=1 the rows are bit for bit those ``stream(window_s, context_s, context_s, dither=False, keep_logp=True)``
        emits; a larger batch may select other kernels by shape and reorder sums (DESIGN.md has the measured difference).
        dither: off by default, so that an alignment is reproducible.
        window_s and context_s ARE STARTING VALUES: nobody has measured accuracy against them on a trained model.
        Memory: T' x C f32 stays on the device - C = 29: 21 MB per hour of audio; C = 4334 (AISHELL): 3.1 GB per hour."""
        wave, duration = self._load_wave(audio_path, resample)
        return self._encode_wave_long(wave, window_s, context_s, int(batch_size), bool(dither)), duration

    def _align_long(self, logp: torch.Tensor, sentences: List[str], duration: float, band: int, max_band: int) -> dict:
        from .align import sentence_records
        sents = [s for s in sentences if s]
        joiner = " " if " " in self.labels else ""
        sentence_ids = [self.text_to_ids(s) for s in sents]
        sep = self.text_to_ids(joiner)
        ids: List[int] = []
        for k, i in enumerate(sentence_ids):
            ids.extend((sep if k else []) + i)
        result = {"duration": duration, "score": 0.0, "band": int(band), "words": [], "sentences": []}
        if not ids:
            return result
        T, S = int(logp.shape[0]), len(ids)
        tg = torch.tensor([ids], dtype=torch.int64, device=logp.device)
        tl = torch.tensor([S], dtype=torch.int32, device=logp.device)
        band, most = int(band), min(int(max_band), ops.CTC_ALIGN_LONG_MAX_BAND)
        while True:
            al = ops.ctc_align_long(logp.unsqueeze(0), tg, None, tl, logp.shape[-1] - 1, band=band) if T else None
            status = int(al.status[0]) if T else 1
            if status == 0:
                break
            if status == 1:
                raise ValueError("align_long: no alignment exists: the transcript (%d labels) is too long for the recording (%d frames)"
                                 % (S, T))
            wider = ops.ctc_align_long_band_at_least(2 * band)     # twice the band, or the next band above that the kernel takes
            if band >= 2 * S + 1 or wider is None or wider > most:
                raise ValueError("align_long: the band of %d states lost every path (max_band %d): the transcript does not follow the "
                                 "recording closely enough, or cannot be spoken on these log-probs at all" % (band, most))
            band = wider
        result["score"], result["band"] = float(al.score[0]), band
        result["words"], result["sentences"] = sentence_records(sentence_ids, al.label_start[0].tolist(), al.label_end[0].tolist(),
                                                                al.frame_logp[0].tolist(), self.labels, self.frame_seconds(), duration,
                                                                sep=len(sep))
        return result

    @torch.no_grad()
    def align_long(self, audio_path, text, band: int = 4096, max_band: int = ops.CTC_ALIGN_LONG_MAX_BAND, **encode) -> dict:
        """Forced alignment of a whole recording (minutes to hours) to its transcript: ``encode_long`` (``**encode`` are its
        keywords), ``text_to_ids``, ``ops.ctc_align_long`` - the Viterbi path inside a band of ``band`` lattice states that
        follows it.  text: a string, or a list of sentences (joined by the space label where the vocabulary has one; empty
        sentences are left out; nothing is normalised, so a sentence should neither start nor end with a space).  Returns {"duration", "score" (the path's log-probability), "band" (the band that aligned),
        "words": the records of ``align``, "sentences": [{"text", "start", "end", "score", "min_word_score", "first_word",
        "n_words"}, ...]} (align.sentence_records), times in seconds of the recording.
        When the band loses every path (status 2 of the kernel) it is doubled (rounded up to the next band the kernel takes), up
        to ``max_band``, whose default is the kernel's widest band, ops.CTC_ALIGN_LONG_MAX_BAND = 8192; above that there is no
        escalation left (a band of 2 S + 1 states or more cannot lose a path: that holds for S <= 4095 only), then ValueError.  ValueError
        also for a transcript with more labels than the recording has frames.  A band narrower than the lattice prunes: it can
        return a feasible path that is not the best one, WITHOUT ANY FLAG - inherent to pruning; low sentence scores are the
        only sign.  The transcript has to cover the whole recording: there is no free start or end."""
        sentences = [text] if isinstance(text, str) else list(text)
        logp, duration = self.encode_long(audio_path, **encode)
        return self._align_long(logp, sentences, duration, band, max_band)

    @torch.no_grad()
    def cut_corpus(self, audio_path, sentences, out_dir: str, manifest_path: str, max_duration: float = 16.7,
                   min_score: Optional[float] = None, band: int = 4096, max_band: int = ops.CTC_ALIGN_LONG_MAX_BAND, prefix: Optional[str] = None,
                   pad_s: float = 0.5, **encode) -> dict:
        """A long recording and its transcript, sentence by sentence -> training utterances: ``align_long``, then consecutive
        sentences are grouped greedily into utterances of at most ``max_duration`` seconds, cut in the middle of the gap between
        neighbouring sentences (``pad_s`` before the first and after the last; align.group_sentences), cut out on the device
        (``ops.gather_segments``) and written to ``out_dir`` as 16-bit PCM wavs ``<prefix>_<index>.wav`` at the parser's sample
        rate (prefix: the audio file's stem).  One line {"audio_filepath", "duration", "text", "score"} per utterance is APPENDED
        to ``manifest_path``, the format ``LibriDataModule`` trains on; score is the lowest word score of the utterance.
        min_score: utterances whose lowest word score is under it are dropped; None (the default) drops nothing - the threshold
        is untuned: nobody has measured it on a trained model.  A sentence longer than max_duration on its own is dropped.
        Returns {"duration", "score", "band", "utterances": the manifest records, "spans": their (start, end) in samples of the
        recording, "dropped": [{"text", "reason"}, ...]}."""
        import wave as wavmod
        from .align import cut_samples, group_sentences
        wave, duration = self._load_wave(audio_path, encode.pop("resample", None))
        logp = self._encode_wave_long(wave, **encode)
        res = self._align_long(logp, [sentences] if isinstance(sentences, str) else list(sentences), duration, band, max_band)
        sents = res["sentences"]
        sr = int(self.audio_parser.sr)
        joiner = " " if " " in self.labels else ""
        groups, too_long = group_sentences(sents, max_duration, min(duration, wave.numel() / float(sr)), joiner, pad_s)
        dropped = [{"text": sents[i]["text"], "reason": "longer than max_duration"} for i in too_long]
        if min_score is not None:
            dropped += [{"text": g["text"], "reason": "min_word_score %.4f under min_score" % g["min_word_score"]}
                        for g in groups if g["min_word_score"] < min_score]
            groups = [g for g in groups if g["min_word_score"] >= min_score]
        spans = cut_samples(groups, sr, int(wave.numel()), max_duration)
        os.makedirs(out_dir, exist_ok=True)
        if prefix is None:
            prefix = os.path.splitext(os.path.basename(audio_path))[0] if isinstance(audio_path, str) else "utt"
        records = []
        for k in range(0, len(groups), 64):                       # 64 utterances per gather: rows as wide as the longest of them
            part = spans[k:k + 64]
            rows, _ = ops.gather_segments(wave, [(0, s, e) for s, e in part])
            pcm = (rows * 32768.0).round().clamp(-32768, 32767).to(torch.int16).cpu().numpy()
            for r, (s, e) in enumerate(part):
                g = groups[k + r]
                path = os.path.join(out_dir, "%s_%05d.wav" % (prefix, g["first"]))
                with wavmod.open(path, "wb") as f:
                    f.setnchannels(1)
                    f.setsampwidth(2)
                    f.setframerate(sr)
                    f.writeframes(pcm[r, :e - s].tobytes())
                records.append({"audio_filepath": path, "duration": (e - s) / float(sr), "text": g["text"], "score": g["min_word_score"]})
        with open(manifest_path, "a", encoding="utf-8") as f:
            for rec in records:
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
        return {"duration": duration, "score": res["score"], "band": res["band"], "utterances": records, "spans": spans, "dropped": dropped}

    # ------------------------------------------------------------------------------------------ streaming
    def stream(self, chunk_s: float = 1.0, left_s: float = 4.0, right_s: float = 1.0, max_segment_s: float = 30.0,
               endpoint_silence_s: Optional[float] = 0.8, dither: bool = True, keep_logp: bool = False):
        """A recogniser for live audio (streaming.StreamingRecognizer): ``feed(samples)`` takes 16 kHz packets of any size and
        returns {"text", "committed", "partial", "frames", "final"} after each, ``finish()`` the final record.  The audio goes
        through overlapping windows of left_s + chunk_s + right_s, each through translate()'s feature chain and forward, and
        the frames of its middle chunk_s through this translator's own decoder (greedy, or the beam search with its LM and
        hotwords as they are now) in its resumable form.  The three context defaults are starting values: nobody has measured
        accuracy against context on a trained model."""
        from .streaming import StreamingRecognizer
        return StreamingRecognizer(self, chunk_s, left_s, right_s, max_segment_s, endpoint_silence_s, dither, keep_logp)

    # ------------------------------------------------------------------------------------------ keyword search
    def _keyword_bank(self, keywords, who: str):
        """keywords (list of str) -> (names, ops.KeywordBank for the model's classes on the translator's device)"""
        if isinstance(keywords, str):
            raise TypeError("%s: keywords is a list of str, not one str" % who)
        names = [str(k) for k in keywords]
        if not names:
            raise ValueError("%s: no keyword" % who)
        n_classes = len(self.labels) + 1                                 # the blank is the model's last class
        return names, ops.build_keywords([self.text_to_ids(k) for k in names], n_classes=n_classes, blank=n_classes - 1,
                                         device=self.device)

    @torch.no_grad()
    def find_keywords(self, audio_path, keywords, threshold: Optional[float] = None, max_hits: int = 8,
                      resample: Optional[bool] = None) -> List[dict]:
        """Where in one audio file is each of `keywords` (a list of str: names, wake words, terms) said?  One record per hit,
        {"keyword", "start", "end", "score", "score_per_label", "confidence"}, sorted by start then keyword order, times in
        seconds.  It searches the model's frame posteriors (``ops.ctc_keyword_search``) instead of the 1-best text, so an
        occurrence off the best path is still found, with a score: the log-likelihood ratio of the phrase over its span against
        the greedy path (0 = the phrase is the greedy path there).  A span is a hit when score >= threshold * (labels of the
        keyword); threshold None is ``ops.ctc_keyword_search``'s default, -2.0 nat per label, a starting value nobody has tuned on a
        trained model - ``keyword_scores`` shows what a recording gives.  Overlapping hits of one keyword keep the best; hits of
        different keywords do not suppress each other.  At most ``max_hits`` hits per keyword are returned.  Works with either
        decoder setting: nothing is decoded.  ValueError for a character outside the vocabulary and for an empty keyword."""
        names, bank = self._keyword_bank(keywords, "find_keywords")
        out, duration = self._encode_file(audio_path, resample)
        logp = out.float().contiguous()
        kw = {} if threshold is None else {"threshold": float(threshold)}
        hits = ops.ctc_keyword_search(logp, None, bank.blank, bank, max_hits=int(max_hits), **kw)
        return hit_records(names, bank.lengths, hits.n_hits[0].tolist(), hits.hit_span[0].tolist(), hits.hit_score[0].tolist(),
                           self.frame_seconds(), duration)

    @torch.no_grad()
    def keyword_scores(self, audio_path, keywords, resample: Optional[bool] = None) -> List[dict]:
        """For choosing a threshold: the best score of every keyword anywhere in the file, whatever the threshold, over its
        labels - one {"keyword", "score_per_label", "start", "end"} per keyword in the order given (-inf and None times for a
        keyword longer than the clip).  ``find_keywords`` with a threshold at or below a keyword's score_per_label reports it."""
        names, bank = self._keyword_bank(keywords, "keyword_scores")
        out, duration = self._encode_file(audio_path, resample)
        hits = ops.ctc_keyword_search(out.float().contiguous(), None, bank.blank, bank, threshold=0.0, max_hits=1)
        return score_records(names, bank.lengths, hits.best_score[0].tolist(), hits.best_span[0].tolist(), self.frame_seconds(), duration)

    @torch.no_grad()
    def find_keywords_long(self, audio_path, keywords, batch_size: int = 32, threshold: Optional[float] = None, max_hits: int = 8,
                           resample: Optional[bool] = None, **vad) -> List[dict]:
        """``find_keywords`` over a recording of any length: cut into utterances on the device as ``translate_long`` cuts it
        (``**vad`` are ``ops.vad_segments``' keywords), the segments encoded in batches of at most ``batch_size``, longest first,
        one keyword search per batch.  The records are ``find_keywords``', times in seconds of the RECORDING, sorted by start then
        keyword order.  Speech outside every segment is not searched, and a phrase that straddles a cut between two segments is
        not found.  ValueError when the recording has more than ``max_segments`` segments, and when a keyword has more than
        ``max_hits`` hits in one segment (naming it): raise max_hits or the threshold."""
        if isinstance(audio_path, str) and not os.path.exists(audio_path):
            raise Exception("音频路径不存在 " + audio_path)
        if int(batch_size) < 1:
            raise ValueError("find_keywords_long: batch_size must be at least 1")
        names, bank = self._keyword_bank(keywords, "find_keywords_long")
        if self._resample(resample):
            y, rate = load_wav_rate(audio_path)
            y = self.audio_parser.resample_to_sr(y, rate)
        else:
            y = load_wav(audio_path)
        if y.shape[1] == 0:
            return []
        wave = y[0].to(self.device).contiguous()
        found = ops.vad_segments(wave, **vad)
        n = int(found.n_segs)
        if n > found.segs.shape[0]:
            raise ValueError("find_keywords_long: the recording has %d segments, more than max_segments=%d" % (n, found.segs.shape[0]))
        segs = [tuple(s) for s in found.segs[:n].tolist()]
        order = sorted(range(n), key=lambda i: segs[i][0] - segs[i][1])  # longest first; equal lengths in time order
        secs, sr = self.frame_seconds(), float(self.audio_parser.sr)
        kw = {} if threshold is None else {"threshold": float(threshold)}
        records: List[dict] = []
        for k in range(0, n, int(batch_size)):
            batch = [segs[i] for i in order[k:k + int(batch_size)]]
            out, t_lens = self._segment_batch(wave, batch)
            hits = ops.ctc_keyword_search(out.float().contiguous(), t_lens.contiguous(), bank.blank, bank, max_hits=int(max_hits), **kw)
            n_hits, span, score = hits.n_hits.tolist(), hits.hit_span.tolist(), hits.hit_score.tolist()
            for b, (s0, s1) in enumerate(batch):
                for j, c in enumerate(n_hits[b]):
                    if c > int(max_hits):
                        raise ValueError("find_keywords_long: the keyword %r has %d hits in the segment %.2f-%.2f s, more than "
                                         "max_hits=%d" % (names[j], c, s0 / sr, s1 / sr, int(max_hits)))
                t0, t1 = s0 / sr, s1 / sr
                for r in hit_records(names, bank.lengths, n_hits[b], span[b], score[b], secs, t1 - t0):
                    r["start"], r["end"] = min(r["start"] + t0, t1), min(r["end"] + t0, t1)     # the recording's time, as _align_batch
                    records.append(r)
        return sort_records(records, names)

    @torch.no_grad()
    def align_manifest(self, manifest: str, out_path: str, batch_size: int = 32) -> List[dict]:
        """Forced alignment of every line of a manifest to its audio, batched over the eval loader (the eval forward of
        evalute_manifest, one ops.ctc_align per batch).  Writes one JSON line per utterance to out_path - audio_filepath, text,
        score (Viterbi log-probability), score_per_frame, words - and returns the records.  An utterance without an alignment
        (transcript too long for its clip) has "words": null and score -inf."""
        if self.resample:
            self._require_16k(manifest, "align_manifest")
        dm = LibriDataModule(train_manifest=manifest, dev_manifest=manifest, test_manifest=manifest, dev_bs=batch_size,
                             num_worker=0, labels=self.labels, device=str(self.model.encoder.native.device),
                             act_dtype=self.model.encoder.native.act_dtype)
        trainer = Trainer(gpus=1, device=str(self.model.encoder.native.device))
        model = self.model
        model.trainer = trainer
        model.eval()
        dm.trainer = trainer
        dm.setup("test")
        loader = dm.test_dataloader()
        durations = dict((d["audio_filepath"], float(d["duration"])) for d in dm.test_datasets.datasets)
        secs = self.frame_seconds()
        records = []
        for batch in trainer._eval_batches(loader, dm, len(loader)):
            out, _, t_lengths, trans, trans_lengths = model._shared(batch)
            logp = out.float().contiguous()
            tg = trans.to(logp.device, torch.int64).contiguous()
            tl = trans_lengths.to(logp.device, torch.int32).contiguous()
            al = ops.ctc_align(logp, tg, t_lengths.contiguous(), tl, logp.shape[-1] - 1)
            score, start, end, flp = al.score.tolist(), al.label_start.tolist(), al.label_end.tolist(), al.frame_logp.tolist()
            tg_h, tl_h, frames = tg.tolist(), tl.tolist(), t_lengths.tolist()
            for b, path in enumerate(batch[-1]):
                ids = tg_h[b][:tl_h[b]]
                rec = {"audio_filepath": path, "text": "".join(self.labels[c] for c in ids), "score": score[b],
                       "score_per_frame": score[b] / max(frames[b], 1), "words": None}
                if math.isfinite(score[b]):
                    rec["words"] = unit_records(ids, start[b], end[b], flp[b], self.labels, secs, durations.get(path))
                records.append(rec)
        with open(out_path, "w", encoding="utf-8") as f:
            for rec in records:
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
        return records
