"""Pseudo-label self-training (the reference's train_ssl.py:223-260 + ssl_codec/utils.py:8-66) on the mel path: the current model
labels an unlabelled manifest, the utterances whose greedy hypothesis is confident enough join the training set until the next
round.  The decode and its confidences are one device op (``ops.greedy_confidence``); only tokens, their counts and the chosen
measure reach the host."""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import ops

logger = logging.getLogger(__name__)

MEASURES = ("ref", "nonblank", "posterior")


@dataclass
class PseudoLabelConfig:
    """start_epoch / every_n_epochs / threshold are the reference's constants (train_ssl.py:224-227,246); nobody has tuned them
    on a trained model of this project.  measure: "ref" = the reference's confidence (minus the mean of the per-frame maxima,
    blank frames included), "nonblank" = the same over the frames whose argmax is a label, "posterior" = minus the log of the
    total probability of the hypothesis per frame (``ops.hyp_neg_logprob``).  Smaller is more confident; an utterance is kept when
    its measure is <= threshold and it has at least min_tokens tokens (0 = the reference, which also injects empty hypotheses).
    batch_size: None = the data module's dev_bs."""
    manifest: object
    start_epoch: int = 300
    every_n_epochs: int = 7
    threshold: float = 0.01
    measure: str = "ref"
    min_tokens: int = 1
    batch_size: Optional[int] = None

    def __post_init__(self):
        if self.measure not in MEASURES:
            raise ValueError("pseudo-label measure must be one of %s, got %r" % (", ".join(MEASURES), self.measure))
        if int(self.every_n_epochs) < 1:
            raise ValueError("pseudo-label every_n_epochs must be at least 1")
        if int(self.min_tokens) < 0:
            raise ValueError("pseudo-label min_tokens must not be negative")


def round_due(epoch: int, cfg: PseudoLabelConfig) -> bool:
    """train_ssl.py:224-227: from start_epoch on, every every_n_epochs-th epoch (counted from 0, not from start_epoch)"""
    return epoch >= cfg.start_epoch and epoch % cfg.every_n_epochs == 0


def confidences(logp: torch.Tensor, lens: Optional[torch.Tensor], blank: int, measure: str = "ref"):
    """(GreedyConfidence, the chosen measure (B,) f32) of a batch of log-probs, all on the device"""
    gc = ops.greedy_confidence(logp, lens, blank)
    if measure == "posterior":
        return gc, ops.hyp_neg_logprob(logp, lens, gc.tokens, gc.n_tokens, blank)
    return gc, gc.conf[:, 0 if measure == "ref" else 1]


@torch.no_grad()
def label_loader(model, trainer, datamodule, loader, cfg: PseudoLabelConfig) -> Tuple[List[dict], Dict[str, float]]:
    """Label every utterance `loader` yields with the model's greedy hypothesis: eval mode, the features made on the device as in
    validation (``trainer._eval_batches``), the weights validation uses (``trainer._eval_params``: the EMA when ema_eval is on).
    Returns (selected, stats): selected = [{"audio_filepath", "duration", "text", "confidence"}, ...] for the utterances with
    confidence <= cfg.threshold and at least cfg.min_tokens tokens; stats = {"pseudo_seen", "pseudo_count", "pseudo_fraction"}."""
    labels = model.labels
    blank = len(labels)
    durations = dict((d["audio_filepath"], d.get("duration")) for d in getattr(getattr(loader, "dataset", None), "datasets", []))
    was_training = bool(getattr(model, "training", False))
    model.eval()
    selected: List[dict] = []
    seen = 0
    on_batch = getattr(trainer, "_pseudo_on_batch", None)      # test hook: (paths, logp, t_lens, GreedyConfidence, measure) per batch
    try:
        with trainer._eval_params(model):
            for batch in trainer._eval_batches(loader, datamodule, len(loader)):
                inputs, pct, paths = batch[0], batch[2], batch[-1]
                out = model._encode(inputs, pct)
                logp = out.float().contiguous()
                t_lens = ops.mask_lengths(pct.to(logp.device, torch.float32).contiguous(), logp.size(1)).contiguous()
                gc, conf = confidences(logp, t_lens, blank, cfg.measure)
                if on_batch is not None:
                    on_batch(paths, logp, t_lens, gc, conf)
                tok_h, n_h, conf_h = gc.tokens.cpu().numpy(), gc.n_tokens.cpu().numpy(), conf.float().cpu().numpy()
                for b, path in enumerate(paths):
                    seen += 1
                    n, c = int(n_h[b]), float(conf_h[b])
                    if c <= cfg.threshold and n >= cfg.min_tokens:
                        selected.append({"audio_filepath": path, "duration": durations.get(path),
                                         "text": "".join(labels[int(k)] for k in tok_h[b, :n]), "confidence": c})
    finally:
        if was_training:
            model.train()
    stats = {"pseudo_seen": float(seen), "pseudo_count": float(len(selected)), "pseudo_fraction": len(selected) / seen if seen else 0.0}
    return selected, stats


def run_round(model, trainer, datamodule, cfg: PseudoLabelConfig) -> Dict[str, float]:
    """One round inside ``Trainer.fit``: label the data module's unlabelled set, inject what passes (replacing the previous
    round's).  world > 1: every rank labels the whole manifest itself - the parameters are identical after the all-reduce - and
    the ranks' counts are compared, so that no rank trains on another set than its peers."""
    dev_bs = datamodule.dev_bs
    try:
        if cfg.batch_size:                     # (the eval ingest sizes its ring by dev_bs)
            datamodule.dev_bs = int(cfg.batch_size)
        selected, stats = label_loader(model, trainer, datamodule, datamodule.pseudo_train_dataloader(), cfg)
    finally:
        datamodule.dev_bs = dev_bs
    if getattr(trainer, "world", 1) > 1:
        v = torch.tensor([stats["pseudo_count"]], dtype=torch.float32, device=trainer.device)
        trainer._all_reduce_sum(v)
        if float(v[0]) != trainer.world * stats["pseudo_count"]:
            raise RuntimeError("pseudo-labelling: this rank selected %d utterances, the %d ranks together %d: the ranks' models or "
                               "data differ" % (int(stats["pseudo_count"]), trainer.world, int(v[0])))
    injected = datamodule.inject_pesudo_datasets(selected)
    logger.info("pseudo labels: %d of %d utterances selected (measure %s <= %g), %d injected", len(selected), int(stats["pseudo_seen"]),
                cfg.measure, cfg.threshold, injected)
    return stats
