"""Inference surface of the reference (predict.py:21-74): checkpoint -> ``AsrTranslator.translate`` and
manifest evaluation, on the HIP path (mel front-end, eval-mode model forward, greedy CTC decode - or, with
``decoder="beam"``, the CTC prefix beam search of beam_search.py, fused with a character n-gram LM when ``lm_path`` names
a text ARPA file).

The checkpoint is the PL-style dict the reference's ``ModelCheckpoint`` writes and ``Trainer`` here
writes too: ``state_dict`` with the reference's key names (``encoder.encoder.block1.seq.0...``) and
``hyper_parameters`` (train.py:194 ``save_hyperparameters``), so reference-trained weights load as-is.
The SSL / LM-beam-search translator (predict.py:76-) belongs to the wav2vec2 branch, out of scope."""
from __future__ import annotations

import time
from typing import List, Optional, Tuple

import torch

from .data_module import AudioParser, LibriDataModule
from .lightning_compat import Trainer
from .train import LightingModule
from . import ops
from .beam_search import BeamSearchDecoderWithLM
from .utils.asr_metrics import WER, word_error_rate

EN_LABELS = [" ", "'"] + [chr(ord("a") + i) for i in range(26)]


class AsrTranslator:
    def __init__(self, model_path: str, map_location: str = "cuda", lang: str = "en", labels: Optional[List[str]] = None,
                 verbose: bool = False, decoder: str = "greedy", beam_width: int = 16, cutoff_top_n: int = 40,
                 cutoff_prob: float = 1.0, lm_path: Optional[str] = None, alpha: float = 1.0, beta: float = 1.0):
        """model_path: a ``.ckpt`` written by the reference or by ``Trainer``; map_location must name a GPU
        ("cuda" / "cuda:0"): there is no CPU path.  ``labels`` overrides the language's vocabulary.
        decoder: "greedy" (argmax + CTC collapse, the default) or "beam" (CTC prefix beam search; with ``lm_path``, a text ARPA
        character LM, fused with it: ``alpha`` weighs the LM, ``beta`` is the per-label bonus)."""
        if decoder not in ("greedy", "beam"):
            raise ValueError("decoder must be 'greedy' or 'beam', got %r" % (decoder,))
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
        self.model = LightingModule.load_from_checkpoint(model_path, map_location=map_location, device=str(map_location))
        self.audio_parser = AudioParser(device=str(map_location))
        self.audio_parser.act_dtype = self.model.encoder.native.act_dtype
        self.device = torch.device(map_location)
        self.wer = WER(vocabulary=self.labels)
        self.decoder = decoder
        self.beam = BeamSearchDecoderWithLM(self.labels, beam_width, alpha, beta, lm_path, 1, cutoff_prob=cutoff_prob,
                                            cutoff_top_n=cutoff_top_n, device=str(map_location))
        self.model.eval()

    @torch.no_grad()
    def translate(self, audio_path) -> str:
        """One local audio file (path or file object) -> text (predict.py:44-63): no dither-free shortcut, the same
        feature chain as training without augmentation, eval-mode BN, argmax, CTC collapse."""
        t0 = time.time()
        inputs = self.audio_parser.parse_audio(audio_path, mask=False)
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
    def translate_nbest(self, audio_path, n: int = 5) -> List[Tuple[str, float]]:
        """One audio file -> the n best beam hypotheses [(text, log-probability), ...], best first (any decoder setting)"""
        inputs = self.audio_parser.parse_audio(audio_path, mask=False)
        pct = torch.ones(inputs.shape[0], dtype=torch.float32, device=self.device)
        out = self.model._encode(inputs, pct)
        return [(text, score) for score, text in self.beam.decode_nbest(out, None, n)[0]]

    def evalute_manifest(self, test_manifest: str, batch_size: int = 32, num_workers: int = 0, decoder: Optional[str] = None):
        """WER over a manifest (predict.py:65-74; the reference's spelling kept).  decoder: None = the translator's own.
        Greedy runs Trainer.test; beam runs the same eval forward and loss, decodes with the beam search and scores its
        top hypothesis.  Both return one record per batch: test_loss, input, test_wer, pred, true, path."""
        decoder = self.decoder if decoder is None else decoder
        if decoder not in ("greedy", "beam"):
            raise ValueError("decoder must be 'greedy' or 'beam', got %r" % (decoder,))
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
