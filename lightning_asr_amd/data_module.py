"""Data contract of the reference's data_module.py with the feature front-end moved to the GPU.

Same public names and arguments: ``MyAudioDataset``, ``AudioParser``, ``LibriDataModule`` (manifest =
JSON lines ``{"audio_filepath","duration","text"}``, scripts/get_libri.py:135).  What differs, by design:
DataLoader workers only decode PCM; dither, pre-emphasis, STFT, mel, dB, SpecAugment zeros, per-utterance
normalisation and pad-to-longest collate run as ONE batched HIP call (csrc/mel.hip) in
``on_after_batch_transfer``, which hands ``training_step`` the reference's 5-tuple
``(inputs (B,1,64,Tmax), targets, input_percentages, target_sizes, paths)`` (data_module.py:248)."""
from __future__ import annotations

import json
import logging
import math
import os
import random
import wave as _wave
from fractions import Fraction
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import _lib, ops
from .lightning_compat import LightningDataModule


def load_wav_rate(path_or_file):
    """16-bit PCM wav -> ((1, L) f32 in [-1, 1), sample rate of the file): what torchaudio.load returns (data_module.py:153)."""
    try:
        with _wave.open(path_or_file, "rb") as w:
            if w.getsampwidth() != 2:
                raise ValueError("only 16-bit PCM wav is supported")
            n, ch, rate = w.getnframes(), w.getnchannels(), w.getframerate()
            pcm = np.frombuffer(w.readframes(n), dtype="<i2").reshape(-1, ch).T
        return torch.from_numpy(pcm[:1].astype(np.float32) / 32768.0), int(rate)
    except (ValueError, _wave.Error, EOFError) as e:
        # flac / 24-bit / float wav (LibriSpeech's native format): the site's `soundfile`, if it has one (the reference's own
        # requirements list it next to torchaudio; not installed in this image).  No torchaudio anywhere in this package.
        if hasattr(path_or_file, "seek"):
            path_or_file.seek(0)                         # a file-like input was partly consumed by the wave reader above
        try:
            import soundfile as sf
        except ImportError:
            raise ValueError("%s: %s (not a 16-bit PCM wav, and no `soundfile` module to decode other formats)" % (path_or_file, e)) from e
        try:
            data, sr = sf.read(path_or_file, dtype="float32", always_2d=True)
        except Exception as e2:                          # soundfile raises RuntimeError / LibsndfileError for what it cannot read
            raise ValueError("%s: neither the wave reader (%s) nor soundfile (%s) can decode it" % (path_or_file, e, e2)) from e2
        return torch.from_numpy(np.ascontiguousarray(data.T[:1])), int(sr)


def load_wav(path_or_file) -> torch.Tensor:
    """16-bit PCM wav -> (1, L) f32 in [-1, 1) (what torchaudio.load returns, data_module.py:153); the file's rate is dropped, as
    the reference drops it - ``load_wav_rate`` keeps it."""
    return load_wav_rate(path_or_file)[0]


SPEED_MAX_TERM = 100          # numerator and denominator of a speed factor: "a ratio of small integers"


def parse_speed_factors(factors) -> List[Fraction]:
    """conf key ``data.speed_perturb`` -> exact ratios.  None / [] = off.  Each factor is read as ``Fraction(str(f))`` (0.9 ->
    9/10, "3/4" -> 3/4), must lie in [0.5, 2] and reduce to integers of at most 100; at most 8 of them (one filter bank).  Anything
    else is a ValueError.  Speed s = a/b is the rate conversion (a, b): the clip becomes b/a as long (DESIGN.md "Resampling")."""
    if factors is None:
        return []
    if isinstance(factors, (str, bytes)) or not hasattr(factors, "__iter__"):
        raise ValueError("data.speed_perturb must be a list of factors, got %r" % (factors,))
    out = []
    for f in factors:
        if isinstance(f, bool) or not isinstance(f, (int, float, str, Fraction)):
            raise ValueError("data.speed_perturb: %r is not a number" % (f,))
        try:
            fr = Fraction(str(f))
        except (ValueError, ZeroDivisionError) as e:
            raise ValueError("data.speed_perturb: %r is not a ratio of integers" % (f,)) from e
        if not (Fraction(1, 2) <= fr <= 2):
            raise ValueError("data.speed_perturb: factor %s is outside [0.5, 2]" % (f,))
        if fr.numerator > SPEED_MAX_TERM or fr.denominator > SPEED_MAX_TERM:
            raise ValueError("data.speed_perturb: factor %s = %s is not a ratio of small integers (<= %d)" % (f, fr, SPEED_MAX_TERM))
        out.append(fr)
    if len(out) > 8:
        raise ValueError("data.speed_perturb: at most 8 factors (one filter bank), got %d" % len(out))
    return out


class WaveAugConfig:
    """conf keys ``data.noise_manifest / noise_prob / noise_snr_db / noise_max_seconds / rir_manifest / rir_prob``, checked.
    A ValueError names the key for a probability outside [0, 1], ``lo > hi``, a non-positive budget."""

    def __init__(self, noise_manifest=None, noise_prob=0.5, noise_snr_db=(5, 20), noise_max_seconds=600, rir_manifest=None, rir_prob=0.3):
        def prob(v, key):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= float(v) <= 1.0):      # (NaN fails the comparison)
                raise ValueError("data.%s must be a probability in [0, 1], got %r" % (key, v))
            return float(v)
        self.noise_manifest = None if noise_manifest in (None, "") else str(noise_manifest)
        self.rir_manifest = None if rir_manifest in (None, "") else str(rir_manifest)
        self.noise_prob, self.rir_prob = prob(noise_prob, "noise_prob"), prob(rir_prob, "rir_prob")
        try:
            lo, hi = (float(v) for v in noise_snr_db)
        except (TypeError, ValueError) as e:
            raise ValueError("data.noise_snr_db must be [lo, hi] in dB, got %r" % (noise_snr_db,)) from e
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
            raise ValueError("data.noise_snr_db must be [lo, hi] with lo <= hi, got %r" % (noise_snr_db,))
        self.noise_snr_db = (lo, hi)
        if isinstance(noise_max_seconds, bool) or not isinstance(noise_max_seconds, (int, float)) or not (float(noise_max_seconds) > 0.0) \
                or not math.isfinite(float(noise_max_seconds)):
            raise ValueError("data.noise_max_seconds must be a positive number of seconds, got %r" % (noise_max_seconds,))
        self.noise_max_seconds = float(noise_max_seconds)

    @property
    def on(self) -> bool:
        return self.noise_manifest is not None or self.rir_manifest is not None


def load_aug_manifest(path: str, key: str, audio_parser, max_seconds: Optional[float] = None) -> List[np.ndarray]:
    """JSON lines with ``audio_filepath`` -> the files as 1-D f32 arrays at the parser's rate (``load_wav_rate``; a file at
    another rate is converted with ``ops.resample``), in manifest order until ``max_seconds`` of audio is held (the file that
    crosses the budget is cut at it).  An empty manifest is a ValueError that names the conf key."""
    out, budget = [], None if max_seconds is None else int(max_seconds * audio_parser.sr)
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            if budget is not None and budget <= 0:
                break
            y = audio_parser.resample_to_sr(*load_wav_rate(json.loads(line)["audio_filepath"]))[0].cpu().numpy()
            if budget is not None:
                y = y[:budget]
                budget -= y.size
            if y.size:
                out.append(np.ascontiguousarray(y, dtype=np.float32))
    if not out:
        raise ValueError("data.%s: %s lists no audio" % (key, path))
    return out


class WaveAug:
    """noise and reverberation of the training clips (DESIGN.md "Noise and reverberation"): the draws on the parser's host
    ``random.Random`` and the device operator, built on first use.  ``rirs`` / ``noises``: lists of 1-D f32 | int16 host arrays,
    either may be empty (that kind is off)."""

    def __init__(self, rirs, noises, rir_prob=0.3, noise_prob=0.5, noise_snr_db=(5, 20), device="cuda"):
        cfg = WaveAugConfig(noise_prob=noise_prob, noise_snr_db=noise_snr_db, rir_prob=rir_prob)
        self.rirs, self.noises, self.device = list(rirs), list(noises), device
        self.rir_prob, self.noise_prob, self.snr = cfg.rir_prob, cfg.noise_prob, cfg.noise_snr_db
        self.noise_lens = [int(len(c)) for c in self.noises]
        self._op = None

    def draw(self, rand) -> tuple:
        """(rir_id, noise_id, noise_start, snr_cdb) of one utterance.  Drawn only when needed: u < rir_prob, the RIR's index,
        u < noise_prob, the clip's index, randrange(len_c), round(100 * uniform(lo, hi)) - a kind that is off draws nothing,
        an index is drawn only after its probability draw passes."""
        rir = nid = -1
        start = snr = 0
        if self.rirs and rand.random() < self.rir_prob:
            rir = rand.randrange(len(self.rirs))
        if self.noises and rand.random() < self.noise_prob:
            nid = rand.randrange(len(self.noises))
            start = rand.randrange(self.noise_lens[nid])
            snr = int(round(100.0 * rand.uniform(*self.snr)))
        return rir, nid, start, snr

    def op(self):
        if self._op is None:
            self._op = ops.WaveAugmenter(self.rirs, self.noises, self.device)
        return self._op


class AudioParser:
    """``parse_audio(path, mask) -> (1, 64, T)`` (data_module.py:150-174), computed on the GPU."""

    def __init__(self, win_len=0.02, sr=16000, device="cuda"):
        if int(win_len * sr) != 320 or sr != 16000:
            raise NotImplementedError("the HIP front-end is built for win_len=0.02, sr=16000 (data_module.py:59)")
        self.win_len, self.sr = win_len, sr
        self.hop_length = int(win_len * sr) // 2          # hop of the mel front-end in samples (data_module.py:66-67)
        self.rand = random.Random()
        self.device = torch.device(device)
        self.speed_factors: List[Fraction] = []           # speed perturbation (LibriDataModule(speed_perturb=...)); [] = off
        self._speed_rs = None
        self.wave_aug: Optional[WaveAug] = None            # noise / reverberation (LibriDataModule(noise_manifest=..., rir_manifest=...)); None = off

    # -- the two random pieces of the training-time chain, drawn on the host like the reference ----
    def sub_secquence(self, x: torch.Tensor, weight: float = 0.1) -> torch.Tensor:
        """Bug-compatible: the slice END is target_length, not location+target_length (:138-148)."""
        length = x.shape[1]
        target_length = int(length * np.random.uniform(weight, 1))
        location = int(np.random.uniform(0, length - target_length))
        return x[:, location:target_length]

    def crop_raw(self, x: torch.Tensor, weight: float = 0.98, lead_in: bool = True):
        """The same two draws applied to the RAW waveform, for the device chain: the reference dithers and pre-emphasises the
        whole clip and slices afterwards (:155-159), so the crop's first sample is ``y[loc] - 0.97 y[loc-1]``.  Returns
        (row, lead): ``row`` = the slice with the sample before it in front when ``loc > 0`` (lead = 1, ``_lib.LEN_LEAD`` in the
        length word handed to the mel kernel), which then produces exactly the reference's values.
        lead_in=False (speed perturbation: the crop is resampled before the mel kernel sees it, and a resampled row has no
        sample "before" it): the bare slice, lead = 0 - its first sample is pre-emphasised as a file's first sample is."""
        length = x.shape[1]
        target_length = int(length * np.random.uniform(weight, 1))
        location = int(np.random.uniform(0, length - target_length))
        lead = 1 if (lead_in and location > 0 and target_length > location) else 0
        return x[:, location - lead:target_length], lead

    # -- speed perturbation (Ko et al. 2015): factor s = a/b is the rate conversion (a, b), the clip becomes b/a as long ----------
    def draw_speed(self) -> int:
        """index of one utterance's factor in ``speed_factors``: drawn after the crop's draws, before the SpecAugment rectangle"""
        return self.rand.randrange(len(self.speed_factors))

    def speed_out_len(self, n: int, k: int) -> int:
        f = self.speed_factors[k]
        return -((-int(n) * f.denominator) // f.numerator)

    def speed_resampler(self):
        """the filter bank of ``speed_factors`` on the parser's device, built on first use"""
        if self._speed_rs is None:
            self._speed_rs = ops.Resampler([(f.numerator, f.denominator) for f in self.speed_factors], self.device)
        return self._speed_rs

    def draw_wave_aug(self) -> tuple:
        """one utterance's (rir_id, noise_id, noise_start, snr_cdb): after its speed factor, before its SpecAugment rectangle"""
        return self.wave_aug.draw(self.rand)

    def perturbs(self, mask: bool) -> bool:
        """a training batch with speed perturbation or noise / reverberation on: its clips are rewritten on the device before the
        mel kernel sees them, so they carry no lead-in sample (a resampled row has no sample "before" it)"""
        return bool(mask) and (bool(getattr(self, "speed_factors", None)) or getattr(self, "wave_aug", None) is not None)

    def draw_speed_batch(self, n: int, mask: bool):
        """one speed factor (index into ``speed_factors``) per utterance of a training batch, None when off or not training.  The
        draws of a DataLoader batch are made in the main process, where the batch reaches the GPU (a worker's copy of `rand` is
        not reseeded per worker): all factors, then all parameter words, then (``draw_aug_batch``) all rectangles"""
        return [self.draw_speed() for _ in range(n)] if mask and getattr(self, "speed_factors", None) else None

    def draw_wave_aug_batch(self, n: int, mask: bool):
        """one (rir_id, noise_id, noise_start, snr_cdb) per utterance of a training batch, None when off or not training"""
        return [self.draw_wave_aug() for _ in range(n)] if mask and getattr(self, "wave_aug", None) is not None else None

    def draw_spec_augment(self, n_time: int, freq_mask: Union[int, float] = 27, time_mask: Union[int, float] = 0.07):
        """(rect_x, w_x, rect_y, w_y) with the draw order of spec_augment (:97-122)."""
        if isinstance(freq_mask, float):
            freq_mask = int(64 * freq_mask)
        if isinstance(time_mask, float):
            time_mask = int(n_time * time_mask)
        w_x = int(self.rand.uniform(0, freq_mask))
        w_y = int(self.rand.uniform(0, time_mask))
        rect_x = int(self.rand.uniform(0, 64 - w_x))
        rect_y = int(self.rand.uniform(0, n_time - w_y))
        return rect_x, w_x, rect_y, w_y

    def spec_augment(self, x: torch.Tensor, freq_mask: Union[int, float] = 27, time_mask: Union[int, float] = 100) -> torch.Tensor:
        """The reference's public method (data_module.py:97-122), same signature and draw order: x (1, 64, T) -> a copy with
        `w_x` mel rows from `rect_x` and `w_y` frames from `rect_y` set to zero.  Inside `parse_audio` / the training loop the same
        rectangle travels into the mel kernel (`draw_spec_augment` + `lasr_mel_fwd`'s aug); this stand-alone form is one
        `lasr_spec_augment` launch on an existing feature tensor."""
        if x.dim() != 3:
            raise ValueError("spec_augment expects (1, F, T) features, got %s" % (tuple(x.shape),))
        if isinstance(freq_mask, float):
            freq_mask = int(x.shape[1] * freq_mask)
        if isinstance(time_mask, float):
            time_mask = int(x.shape[2] * time_mask)
        w_x = int(self.rand.uniform(0, freq_mask))
        w_y = int(self.rand.uniform(0, time_mask))
        rect_x = int(self.rand.uniform(0, x.shape[1] - w_x))
        rect_y = int(self.rand.uniform(0, x.shape[2] - w_y))
        xin = x.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(xin)
        aug = torch.tensor([[rect_x, w_x, rect_y, w_y]] * xin.shape[0], dtype=torch.int32, device=self.device)
        ops.call("lasr_spec_augment", xin.data_ptr(), out.data_ptr(), aug.data_ptr(), xin.shape[0], xin.shape[1], xin.shape[2],
                 torch.cuda.current_stream(self.device).cuda_stream)
        return out.to(x.device)

    def resample_to_sr(self, y: torch.Tensor, rate: int) -> torch.Tensor:
        """(1, L) f32 host wave at `rate` -> (1, n_out) f32 at the parser's rate, converted on the device (``ops.resample``,
        DESIGN.md "Resampling"); a wave already at that rate is returned as it is"""
        if int(rate) == self.sr:
            return y
        return ops.resample(y[0].to(self.device), int(rate), self.sr)[0].unsqueeze(0)

    def parse_audio(self, audio_path, mask=False, resample=False) -> torch.Tensor:
        """resample=True: a file whose sample rate is not 16000 is converted to it on the device before the feature chain;
        resample=False (the default, and the reference's behaviour) feeds the samples as they are, whatever the file's rate."""
        if isinstance(audio_path, str) and not os.path.exists(path=audio_path):
            raise Exception("音频路径不存在 " + audio_path)
        if resample:
            y = self.resample_to_sr(*load_wav_rate(audio_path))
        else:
            y = load_wav(audio_path)
        lead = 0
        if mask:
            y, lead = self.crop_raw(y, weight=0.98)
        return self.features_one(y, mask, lead)[0]

    def features_one(self, y: torch.Tensor, mask: bool = False, lead: int = 0):
        """``features([y[0]], mask, leads=[lead])`` for one (1, L) wave; a wave that already sits on the device (a resampled file)
        stays there: the same mel call on the same row, without the trip through the pinned staging buffer"""
        if not y.is_cuda or mask or lead or y.shape[1] == 0:
            return self.features([y[0]], mask, leads=[lead])
        lens = torch.full((1,), y.shape[1], dtype=torch.int32, device=y.device)
        return self.features_device(y.contiguous(), lens, None, True, logical_len=y.shape[1])

    # ---- the batched device front-end ---------------------------------------------------------------------------------------
    def device_dither(self):
        """``y += 1e-5 * randn_like(y)`` (:155) is drawn inside the mel kernel (Philox keyed by the process seed)"""
        if getattr(self, "_dither", None) is None:
            self._dither = ops.DeviceDither(int(torch.initial_seed()), self.device)
        return self._dither

    def draw_aug_batch(self, sample_lens) -> torch.Tensor:
        """(B, 4) int32 SpecAugment rectangles for utterances of `sample_lens` samples (host draws, as the reference)"""
        return torch.tensor([self.draw_spec_augment(1 + (int(l) + 64) // 160) for l in sample_lens], dtype=torch.int32)

    def features_device(self, wave: torch.Tensor, lens: Optional[torch.Tensor], aug: Optional[torch.Tensor] = None, dither: bool = True,
                        logical_len: Optional[int] = None):
        """wave (B, L) f32 or int16 PCM ALREADY in HBM -> (inputs (B,1,64,Tmax) f32 with its channels-last twin attached,
        input_percentages (B,)); frames past each utterance are zero (collate, :222-248).  logical_len: the longest utterance when
        the rows are wider than that - Tmax is ITS frame count (the reference pads to the longest feature matrix)."""
        bft, btf, frames, pct = ops.mel(wave, lens, self.device_dither() if dither else None, aug, True, self._act_dtype(),
                                        logical_len=logical_len)
        inputs = bft.unsqueeze(1)
        inputs._lasr_btf = btf                                           # channels-last twin for the model
        return inputs, pct

    def _staging(self, n: int) -> torch.Tensor:
        """two alternating pinned f32 staging buffers, reused across batches (a buffer is rewritten only after its last H2D copy
        has completed)"""
        st = getattr(self, "_stage", None)
        if st is None:
            st = self._stage = {"buf": [None, None], "ev": [None, None], "k": 0}
        k = st["k"] = st["k"] ^ 1
        if st["ev"][k] is not None:
            st["ev"][k].synchronize()
        if st["buf"][k] is None or st["buf"][k].numel() < n:
            st["buf"][k] = torch.empty(int(n * 1.25) + 1024, dtype=torch.float32).pin_memory()
        return st["buf"][k][:n]

    @staticmethod
    def check_no_lead(leads, speed, wave_aug) -> None:
        """a wave that is resampled or augmented on the device has no sample "before" it: a lead-in sample is a caller error"""
        kind = "a speed-perturbed" if speed is not None else "an augmented" if wave_aug is not None else None
        if kind and leads is not None and any(int(l) for l in leads):
            raise ValueError(kind + " wave cannot carry a lead-in sample")

    def wave_chain(self, waves: Sequence[torch.Tensor], leads: Optional[Sequence[int]] = None, speed: Optional[Sequence[int]] = None,
                   wave_aug: Optional[Sequence[tuple]] = None, device=None):
        """list of (L_i,) f32 host waves -> (rows (B, L) f32 on the GPU, length words (B,) int32 on the host, samples per utterance):
        padded into a reused pinned buffer, ONE H2D copy for the batch.  leads[i] = 1: waves[i] starts with a lead-in sample
        (``crop_raw``), flagged in its length word and not counted as a sample.
        speed[i]: index into ``speed_factors`` - the uploaded batch is resampled on the device (f32 -> f32), and every length is
        the resampled one.  wave_aug[i]: (rir_id, noise_id, noise_start, snr_cdb) - reverberation and noise on the device
        (f32 -> f32) directly after the resampler; the lengths do not change.  Such waves carry no lead-in sample."""
        self.check_no_lead(leads, speed, wave_aug)
        B = len(waves)
        L = max(int(w.numel()) for w in waves)
        host = self._staging(B * L).view(B, L)
        host.zero_()
        for i, w in enumerate(waves):
            host[i, :w.numel()] = w.cpu() if w.is_cuda else w
        leads = [int(l) for l in leads] if leads is not None else [0] * B
        n_out = [w.numel() - ld for w, ld in zip(waves, leads)]
        lens = torch.tensor([n | (_lib.LEN_LEAD if ld else 0) for n, ld in zip(n_out, leads)], dtype=torch.int32)
        dev = self.device if device is None else torch.device(device)     # where the rows go: the caller's device, else the parser's
        wave = host.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._stage["ev"][self._stage["k"]] = ev
        if speed is not None:
            n_out = [self.speed_out_len(n, int(k)) for n, k in zip(n_out, speed)]
            wave, _ = self.speed_resampler()(wave, lens.to(dev), torch.tensor([int(k) for k in speed], dtype=torch.int32).to(dev),
                                             L_out=max(max(n_out), 1))
            lens = torch.tensor(n_out, dtype=torch.int32)
        if wave_aug is not None:
            wave, _, _ = self.wave_aug.op()(wave, lens.to(dev), torch.tensor([list(p) for p in wave_aug], dtype=torch.int32).to(dev))
        return wave, lens, n_out

    def features(self, waves: Sequence[torch.Tensor], mask: bool, dither: bool = True, leads: Optional[Sequence[int]] = None,
                 speed: Optional[Sequence[int]] = None, wave_aug: Optional[Sequence[tuple]] = None):
        """list of (L_i,) f32 host waves -> (inputs, input_percentages) on the GPU: ``wave_chain``, the SpecAugment rectangles
        drawn for the lengths it returns, then ``features_device``"""
        wave, lens, n_out = self.wave_chain(waves, leads, speed, wave_aug)
        aug = self.draw_aug_batch(n_out).to(self.device) if mask else None
        # Tmax = the frames of the longest UTTERANCE (a row's lead-in sample is not part of it: it emits no frame of its own)
        return self.features_device(wave, lens.to(self.device), aug, dither, logical_len=max(max(n_out), 1))

    def _act_dtype(self):
        return getattr(self, "act_dtype", torch.float32)


class MyAudioDataset(Dataset):
    def __init__(self, manifest_path: list, labels, max_duration=16.7, mask=False, win_len=0.02, sr=16000, text_optional=False):
        """text_optional: a manifest line without "text" is an utterance with the empty transcript (the unlabelled manifest of
        pseudo-labelling, ``LibriDataModule(pesudo_manifest=...)``); everywhere else such a line fails where its text is read"""
        self.datasets = []
        self.labels = labels
        self.mask = mask
        for item in manifest_path:
            total_count, total_duration = 0, 0.0
            with open(item, encoding="utf-8") as f:
                for line in f.readlines():
                    if not line.strip():
                        continue
                    data = json.loads(line)
                    if data["duration"] > max_duration:
                        total_count += 1
                        total_duration += data["duration"]
                        continue
                    if text_optional:
                        data.setdefault("text", "")
                    self.datasets.append(data)
            logging.info("过滤音频条数:{:d}条".format(total_count))
            logging.info("过滤音频时长:{:.2f}分钟".format(total_duration / 60))
        self.index2char = dict((i, labels[i]) for i in range(len(labels)))
        self.char2index = dict((labels[i], i) for i in range(len(labels)))

    def __getitem__(self, index):
        """-> (wave (L,) f32 on the host, token ids, path): PCM decode only, features are batched on the GPU."""
        data = self.datasets[index]
        text2id = [self.char2index[char] for char in data["text"]]
        return load_wav(data["audio_filepath"])[0], text2id, data["audio_filepath"]

    def id2txt(self, id_list):
        for id in id_list:
            if id >= len(self.index2char):
                raise Exception("index out of the lengths请检查id的大小范围")
        return "".join(self.index2char[id] for id in id_list)

    def __len__(self):
        return len(self.datasets)


class BucketBatchSampler(torch.utils.data.Sampler):
    """Length-bucketed batches (BASELINE config 5; not in the reference, which pads to the batch's
    longest clip, data_module.py:225-230): utterances are sorted by duration inside shuffled mega-chunks
    of ``bucket_batches`` batches, so padding inside a batch stays small; batch order is reshuffled
    every epoch.  Data-parallel ranks take disjoint batches (rank::world)."""

    def __init__(self, durations, batch_size: int, bucket_batches: int = 50, shuffle: bool = True, drop_last: bool = True,
                 seed: int = 0, rank: int = 0, world: int = 1):
        self.durations = list(durations)
        self.batch_size, self.bucket_batches = batch_size, bucket_batches
        self.shuffle, self.drop_last, self.seed, self.rank, self.world = shuffle, drop_last, seed, rank, world
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _batches(self):
        n = len(self.durations)
        rng = random.Random(self.seed + self.epoch)
        idx = list(range(n))
        if self.shuffle:
            rng.shuffle(idx)
        chunk = self.batch_size * self.bucket_batches
        batches = []
        for i in range(0, n, chunk):
            part = sorted(idx[i:i + chunk], key=lambda j: self.durations[j])
            for k in range(0, len(part), self.batch_size):
                b = part[k:k + self.batch_size]
                if len(b) == self.batch_size or not self.drop_last:
                    batches.append(b)
        if self.shuffle:
            rng.shuffle(batches)
        usable = len(batches) - len(batches) % self.world if self.world > 1 else len(batches)
        return batches[:usable][self.rank::self.world]

    def __iter__(self):
        return iter(self._batches())

    def __len__(self):
        return len(self._batches())


def _rebuild_wave_batch(items, leads):
    wb = WaveBatch(items)
    wb.leads = leads
    return wb


class WaveBatch(tuple):
    """(waves list, targets (B,Smax) int64, target_sizes (B) int32, paths, mask flag) from the workers.  ``leads`` (list of 0/1,
    or None): waves[i] starts with a lead-in sample (``AudioParser.crop_raw``); it survives the DataLoader's pickling."""
    leads = None

    def __reduce__(self):
        return (_rebuild_wave_batch, (tuple(self), self.leads))


class LibriDataModule(LightningDataModule):
    def __init__(self, train_manifest, dev_manifest, test_manifest, labels: list, train_bs=16, dev_bs=16, num_worker=0,
                 train_max_duration=16.7, dev_max_duration=40, device="cuda", act_dtype=torch.float32,
                 bucket_by_length: bool = False, bucket_batches: int = 50, train_crop: bool = True, speed_perturb=None,
                 noise_manifest=None, noise_prob=0.5, noise_snr_db=(5, 20), noise_max_seconds=600, rir_manifest=None, rir_prob=0.3,
                 pesudo_manifest=None):
        super().__init__()
        as_list = lambda m: list(m) if isinstance(m, (list, tuple)) else [m]  # noqa: E731
        self.train_manifest, self.dev_manifest, self.test_manifest = as_list(train_manifest), as_list(dev_manifest), as_list(test_manifest)
        # the unlabelled manifest of pseudo-label self-training (the reference's spelling, conf/ssl-conf.yaml / train_ssl.py:357;
        # conf key data.pesudo_manifest, null = off): lines need "audio_filepath" and "duration" only
        self.pesudo_manifest = as_list(pesudo_manifest) if pesudo_manifest else None
        self.pesudo_train_datasets = None
        self._train_base, self._pesudo_injected = None, []
        self.train_bs, self.dev_bs = train_bs, dev_bs
        self.labels = labels
        self.num_worker = num_worker
        self.train_max_duration, self.dev_max_duration = train_max_duration, dev_max_duration
        self.audio_parser = AudioParser(device=device)
        self.audio_parser.act_dtype = act_dtype
        self.bucket_by_length = bool(bucket_by_length)       # BASELINE cfg5: length-bucketed batches (conf key data.bucket_by_length)
        self.bucket_batches = int(bucket_batches)            # batches per sorted mega-chunk (conf key data.bucket_batches)
        self.train_crop = bool(train_crop)                   # the reference's random sub-sequence of every training clip (data_module.py:158-159); conf key data.train_crop
        # speed perturbation of every training clip (conf key data.speed_perturb: a list of factors, [] / absent = off): one factor
        # per utterance, applied on the device by ops.Resampler on every route that yields training batches
        self.speed_perturb = parse_speed_factors(speed_perturb)
        self.audio_parser.speed_factors = self.speed_perturb
        # additive noise at a drawn SNR and reverberation with a drawn RIR (conf keys data.noise_* / data.rir_*; a null manifest =
        # that kind off): per training utterance, on the device directly after the resampler, on every route that yields training batches
        self.wave_aug_cfg = WaveAugConfig(noise_manifest, noise_prob, noise_snr_db, noise_max_seconds, rir_manifest, rir_prob)

    def setup_wave_aug(self):
        """reads the noise and RIR manifests ONCE and hands the parser its ``WaveAug`` (with both manifests null the parser keeps
        what it has: None unless a caller put one there)"""
        cfg = self.wave_aug_cfg
        if cfg.on and self.audio_parser.wave_aug is None:
            ap = self.audio_parser
            noises = load_aug_manifest(cfg.noise_manifest, "noise_manifest", ap, cfg.noise_max_seconds) if cfg.noise_manifest else []
            rirs = load_aug_manifest(cfg.rir_manifest, "rir_manifest", ap) if cfg.rir_manifest else []
            ap.wave_aug = WaveAug(rirs, noises, cfg.rir_prob, cfg.noise_prob, cfg.noise_snr_db, ap.device)

    def setup(self, stage=None):
        self.speed_perturb = parse_speed_factors(self.speed_perturb)     # (a list assigned after construction is checked here)
        self.audio_parser.speed_factors = self.speed_perturb
        self.setup_wave_aug()
        self.train_datasets = MyAudioDataset(self.train_manifest, self.labels, mask=True, max_duration=self.train_max_duration)
        self.dev_datasets = MyAudioDataset(self.dev_manifest, self.labels, max_duration=self.dev_max_duration)
        self.test_datasets = MyAudioDataset(self.test_manifest, self.labels, max_duration=self.dev_max_duration)
        self._train_base, self._pesudo_injected = list(self.train_datasets.datasets), []
        if self.pesudo_manifest:           # ssl_data_module.py:240: the unlabelled clips are cut at the DEV duration
            self.pesudo_train_datasets = MyAudioDataset(self.pesudo_manifest, self.labels, max_duration=self.dev_max_duration,
                                                        text_optional=True)

    # ---- pseudo-label self-training (ssl_data_module.py:232-281) ------------------------------------------------------------------
    def pseudo_train_dataloader(self):
        """the unlabelled clips in manifest order with the eval collate (the reference shuffles them: only the order differs)"""
        if self.pesudo_train_datasets is None:
            raise RuntimeError("pseudo_train_dataloader: the data module was built without pesudo_manifest (or setup() has not run)")
        return self._loader(self.pesudo_train_datasets, self.dev_bs, False)

    def inject_pesudo_datasets(self, datas) -> int:
        """The pseudo-labelled clips of one round join the training set: `datas` is the reference's [(audio_path, text), ...] or a
        list of {"audio_filepath", "text", "duration"?, ...} (pseudo_label.label_loader).  They REPLACE the previous round's and
        stay until the next call; train_dataloader() then serves original + injected.  Dropped with a warning: an entry whose file
        is missing (as the reference does), and - unlike the reference, which injects them and lets the batch grow - one longer
        than train_max_duration or with a character outside the labels.  Returns the number injected."""
        if self._train_base is None:
            raise RuntimeError("inject_pesudo_datasets: setup() has not run")
        known = dict((d["audio_filepath"], d.get("duration")) for d in self.pesudo_train_datasets.datasets) \
            if self.pesudo_train_datasets is not None else {}
        c2i = self.train_datasets.char2index
        kept, missing, too_long, bad_text = [], 0, 0, 0
        for item in datas:
            if isinstance(item, dict):
                rec = dict(item)
            else:
                path, text = item
                rec = {"audio_filepath": path, "text": text}
            path = rec["audio_filepath"]
            if not os.path.exists(path):
                logging.warning("伪标签音频路径不存在 " + str(path))
                missing += 1
                continue
            if rec.get("duration") is None:
                dur = known.get(path)
                if dur is None:
                    from .ingest import wav_info
                    frames, _ch, rate, _bits = wav_info(path)
                    dur = frames / float(rate)
                rec["duration"] = float(dur)
            if self.train_max_duration and rec["duration"] > self.train_max_duration:
                too_long += 1
                continue
            if any(ch not in c2i for ch in rec["text"]):
                bad_text += 1
                continue
            kept.append(rec)
        if missing or too_long or bad_text:
            logging.warning("pseudo labels dropped: %d missing files, %d longer than train_max_duration, %d with unknown characters",
                            missing, too_long, bad_text)
        self._pesudo_injected = kept
        ds = self.train_datasets
        ds.datasets = self._train_base + kept
        for cached in ("_lasr_ids_cache", "_lasr_fast_ingest_ok"):      # per-entry caches of the native ingest: the entries changed
            ds.__dict__.pop(cached, None)
        return len(kept)

    def _loader(self, ds, bs, train, distributed=None):
        if train and getattr(self, "bucket_by_length", False):
            world, rank = distributed if distributed is not None else (1, 0)
            bs_ = BucketBatchSampler([d["duration"] for d in ds.datasets], bs, bucket_batches=self.bucket_batches, rank=rank, world=world)
            return DataLoader(ds, batch_sampler=bs_, num_workers=self.num_worker, collate_fn=self._collate_train)
        sampler = None
        if distributed is not None:
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(ds, num_replicas=distributed[0], rank=distributed[1], shuffle=train, drop_last=train)
        collate = self._collate_train if train else self._collate_eval
        return DataLoader(ds, batch_size=bs, num_workers=self.num_worker, pin_memory=False, collate_fn=collate, drop_last=train,
                          shuffle=train and sampler is None, sampler=sampler)

    def train_dataloader(self, distributed=None):
        return self._loader(self.train_datasets, self.train_bs, True, distributed)

    def val_dataloader(self):
        return self._loader(self.dev_datasets, self.dev_bs, False)

    def test_dataloader(self):
        return self._loader(self.test_datasets, self.dev_bs, False)

    def get_train_step(self):
        return len(self.train_dataloader())

    # ---- host half of the collate: ragged waves + padded targets (data_module.py:231-247) ---------
    def _collate_wave(self, batch, mask: bool) -> WaveBatch:
        waves = [b[0] for b in batch]
        leads = None
        if mask and getattr(self, "train_crop", True):   # training-time random sub-sequence (data_module.py:158-159)
            ap = self.audio_parser
            cr = [ap.crop_raw(w.unsqueeze(0), weight=0.98, lead_in=not ap.perturbs(mask)) for w in waves]
            waves, leads = [c[0][0] for c in cr], [c[1] for c in cr]
        max_trans = max(len(b[1]) for b in batch)
        targets = torch.zeros(len(batch), max_trans, dtype=torch.int64)
        target_sizes = torch.zeros(len(batch), dtype=torch.int32)
        for i, b in enumerate(batch):
            target_sizes[i] = len(b[1])
            targets[i, :len(b[1])] = torch.tensor(b[1], dtype=torch.int64)
        wb = WaveBatch((waves, targets, target_sizes, [b[2] for b in batch], mask))
        wb.leads = leads
        return wb

    def _collate_train(self, batch):
        return self._collate_wave(batch, True)

    def _collate_eval(self, batch):
        return self._collate_wave(batch, False)

    _collate_fn = _collate_eval

    def draw_speed_batch(self, n: int, mask: bool):
        return self.audio_parser.draw_speed_batch(n, mask)

    def draw_wave_aug_batch(self, n: int, mask: bool):
        return self.audio_parser.draw_wave_aug_batch(n, mask)

    # ---- device half: ONE batched HIP mel call -> the reference's 5-tuple -------------------------
    def on_after_batch_transfer(self, batch, dataloader_idx=0):
        if not isinstance(batch, WaveBatch):
            return batch
        waves, targets, target_sizes, paths, mask = batch
        speed = self.draw_speed_batch(len(waves), mask)                 # after the crop's draws (collate), before the rectangles (features)
        wave_aug = self.draw_wave_aug_batch(len(waves), mask)           # after the speed factors, before the rectangles
        inputs, pct = self.audio_parser.features(waves, mask, leads=batch.leads, speed=speed, wave_aug=wave_aug)
        dev = inputs.device
        return inputs, targets.to(dev), pct, target_sizes.to(dev), paths
