"""Streaming recognition: audio in packets of any size -> partial and committed text while the speaker is still talking.

The shipped encoders see seconds of context on either side of a frame (symmetric depthwise kernels of 33 to 87 taps over 15 to
52 units), so the encoder side is buffered windows, not cached layer state: ``plan_windows`` cuts the audio received so far into
overlapping windows, each is run through the feature chain and the model on its own, and only the frames in the middle of a
window, which have ``left`` of audio before them and ``right`` after them, are emitted.  The emitted log-prob rows go to the
translator's own decoder in its resumable form (``ops.CtcBeamStream`` from ``BeamSearchDecoderWithLM.open_stream``, or
``ops.GreedyStream``), which gives after every chunk the hypothesis as if the audio ended there.

The plan depends on the number of samples received and on (chunk, left, right) alone, never on how the audio was cut into
packets: the same recording gives the same log-prob rows and the same text whatever the packet size (dither off; with dither the
noise drawn per window differs).

Not done here (DESIGN.md "Streaming recognition"): several live streams in one forward, word timestamps on partials, resampling
of streamed audio (16 kHz in), stability smoothing of partials."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

HOP = 160                     # samples per feature frame
STRIDE = 2                    # feature frames per output frame (every shipped variant)
FRAME = HOP * STRIDE          # samples per output frame: chunk, left and right are multiples of it


def mel_frames(n_samples: int) -> int:
    """feature frames of n_samples samples (lasr_mel_num_frames)"""
    return 1 + (int(n_samples) + 64) // HOP


def default_out_frames(n_mel: int) -> int:
    """output frames of n_mel feature frames (lasr_model_out_frames: the one stride-2 convolution of 33 taps, padding 16)"""
    return (int(n_mel) + 2 * 16 - 33) // 2 + 1


def plan_windows(total_samples_so_far: int, final: bool, chunk: int, left: int, right: int, emitted_frames: int,
                 out_frames: Callable[[int], int] = default_out_frames) -> List[Tuple[int, int, int, int]]:
    """The windows that can be processed now: [(s0, s1, first_out_frame, n_out_frames), ...].  A window is the samples [s0, s1)
    of the recording; of the model's output frames for it, the n_out_frames from first_out_frame on (an index into THAT output)
    are emitted, and they are the recording's frames s0 / 320 + first_out_frame onwards.  Pure: no torch, no state.

    chunk, left, right: samples, multiples of 320 (hop 160 x stride 2), chunk > 0.  Step k is ready once (k + 1) * chunk + right
    samples have arrived; its window is [max(0, k * chunk - left), (k + 1) * chunk + right) and it emits the frames
    [k * chunk / 320, (k + 1) * chunk / 320).  emitted_frames: the frames emitted so far, i.e. where the next step starts.
    final: the recording has ended at total_samples_so_far; after the ready steps one last window takes the rest,
    [max(0, k * chunk - left), total), and emits every remaining frame of it: out_frames(mel_frames(its samples)) of them in
    all (where that window would hold no samples - left = right = 0 and the recording ends on a step - it starts one frame
    earlier).  Nothing is planned for a recording of no samples, or once the last window has been emitted."""
    total, chunk, left, right, emitted = int(total_samples_so_far), int(chunk), int(left), int(right), int(emitted_frames)
    if chunk <= 0 or chunk % FRAME or left < 0 or left % FRAME or right < 0 or right % FRAME:
        raise ValueError("chunk %d (> 0), left %d and right %d (>= 0) must be multiples of %d samples" % (chunk, left, right, FRAME))
    if total < 0 or emitted < 0:
        raise ValueError("negative sample or frame count")
    per = chunk // FRAME
    if emitted % per:
        return []                 # only the last window leaves a partial step behind: the recording is done
    windows = []
    k = emitted // per
    while (k + 1) * chunk + right <= total:
        s0 = max(0, k * chunk - left)
        windows.append((s0, (k + 1) * chunk + right, (k * chunk - s0) // FRAME, per))
        k += 1
    if final and total > 0:
        s0 = max(0, k * chunk - left)
        if s0 == total:           # left = right = 0 and the recording ends on a step: the frame centred on its last sample is
            s0 -= FRAME           # still to come, and its window starts one frame earlier so as to hold samples at all
        first = (k * chunk - s0) // FRAME
        n = out_frames(mel_frames(total - s0)) - first
        if n > 0:
            windows.append((s0, total, first, n))
    return windows


def total_frames(total_samples: int, out_frames: Callable[[int], int] = default_out_frames) -> int:
    """the frames a finished recording of total_samples emits in all: the model's output frames of the whole of it"""
    return out_frames(mel_frames(total_samples)) if total_samples > 0 else 0


def join_texts(texts, labels) -> str:
    """segment texts joined as translate_long joins them (" " where the vocabulary has a space label); empty ones are left out"""
    return (" " if " " in labels else "").join(t for t in texts if t)


class StreamingRecognizer:
    """Built by ``AsrTranslator.stream``.  ``feed(samples)`` takes the next packet of 16 kHz audio and returns
    {"text": committed + partial, "committed", "partial", "frames", "final": False}; ``finish()`` processes what is left, returns
    the same record with "final": True (and "segments": the committed pieces with their frame spans; with keep_logp, "logp": the
    emitted log-prob rows) and resets the recogniser for the next recording.

    chunk_s / left_s / right_s: a step's new audio and the context a window has before and after it, rounded to whole output
    frames (0.02 s).  Latency is chunk_s + right_s plus the compute.  THE DEFAULTS (1.0 / 4.0 / 1.0) ARE STARTING VALUES: nobody
    has measured accuracy against context on a trained model.  Every window is normalised over its own frames, as
    translate_long's rows are.
    max_segment_s: after that many seconds of frames the best hypothesis is committed and the decoder starts over (the beam's
    trie is sized for it).  endpoint_silence_s: the decoder also commits when the emitted frames of that long at the end of a
    step are all blank by argmax while the partial is non-empty (None or 0: off).  The windows go on unchanged across both."""

    def __init__(self, translator, chunk_s: float = 1.0, left_s: float = 4.0, right_s: float = 1.0, max_segment_s: float = 30.0,
                 endpoint_silence_s: Optional[float] = 0.8, dither: bool = True, keep_logp: bool = False):
        import torch
        from .predict import MIN_ROW_SAMPLES
        self.tr = translator
        self.device = translator.device
        sr = float(translator.audio_parser.sr)
        if int(sr) != 16000 or translator.audio_parser.hop_length != HOP:
            raise ValueError("streaming takes 16 kHz audio at hop %d" % HOP)
        native = translator.model.encoder.native
        self._out_frames = lambda n_mel: int(native.out_frames(int(n_mel)))
        if self._out_frames(2 * 4096 + 1) - self._out_frames(4096 + 1) != 4096 // STRIDE:
            raise ValueError("streaming is written for a model of time stride %d" % STRIDE)
        to_samples = lambda s: int(round(float(s) * sr / FRAME)) * FRAME
        self.chunk, self.left, self.right = to_samples(chunk_s), to_samples(left_s), to_samples(right_s)
        if self.chunk <= 0 or self.left < 0 or self.right < 0:
            raise ValueError("chunk_s must be at least one frame (%.2f s), left_s and right_s not negative" % (FRAME / sr))
        self.seg_frames = int(round(float(max_segment_s) * sr / FRAME))
        if self.seg_frames < 1:
            raise ValueError("max_segment_s must be at least one frame")
        self.ep_frames = int(round(float(endpoint_silence_s) * sr / FRAME)) if endpoint_silence_s else 0
        self.dither, self.keep_logp = bool(dither), bool(keep_logp)
        self.blank = len(translator.labels)
        self._min_row = MIN_ROW_SAMPLES
        self._span = self.left + self.chunk + self.right
        self._buf = torch.zeros(2 * self._span + FRAME, dtype=torch.float32, device=self.device)   # the last left + chunk + right of audio
        if translator.decoder == "beam":
            self.decoder = translator.beam.open_stream(1, self.seg_frames)
        else:
            from . import ops
            self.decoder = ops.GreedyStream(1, self.blank, self.seg_frames, device=self.device)
        self.reset()

    def reset(self) -> None:
        """forget the recording so far"""
        self._base = 0            # the recording's sample index of _buf[0]
        self._n = 0               # samples held in _buf
        self._total = 0
        self.frames = 0           # frames emitted
        self._seg_start = 0       # the current segment's first frame
        self._trailing_blank = 0
        self._committed: List[dict] = []
        self._partial = ""
        self._kept = []
        self.decoder.reset()

    # ------------------------------------------------------------------------------------------ audio in
    def _as_wave(self, samples):
        import numpy as np
        import torch
        if isinstance(samples, np.ndarray):
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        elif not torch.is_tensor(samples):
            samples = torch.as_tensor(samples)
        samples = samples.reshape(-1)
        if samples.dtype == torch.int16:
            return samples.to(self.device).to(torch.float32) / 32768.0
        if samples.dtype != torch.float32:
            raise TypeError("streamed audio must be float32 in [-1, 1) or int16 PCM, got %s" % samples.dtype)
        return samples.to(self.device)

    def _append(self, piece) -> None:
        """piece into the buffer, dropping first what no later window reads: the samples before the next step's left context"""
        need_from = max(0, (self.frames // (self.chunk // FRAME)) * self.chunk - self.left - FRAME)   # - FRAME: plan_windows' last window
        drop = min(max(need_from - self._base, 0), self._n)
        if drop and self._n + piece.numel() > self._buf.numel():
            self._buf[:self._n - drop] = self._buf[drop:self._n].clone()
            self._base += drop
            self._n -= drop
        self._buf[self._n:self._n + piece.numel()] = piece
        self._n += piece.numel()
        self._total += piece.numel()

    # ------------------------------------------------------------------------------------------ windows
    def _window_logp(self, s0: int, s1: int, first: int, n: int):
        """the emitted log-prob rows (n, C) f32 of the window [s0, s1)"""
        import torch
        tr = self.tr
        length = s1 - s0
        row = torch.zeros(1, max(length, self._min_row), dtype=torch.float32, device=self.device)
        row[0, :length] = self._buf[s0 - self._base:s1 - self._base]
        lens = torch.full((1,), length, dtype=torch.int32, device=self.device)
        inputs, pct = tr.audio_parser.features_device(row, lens, None, self.dither, logical_len=row.shape[1])
        out = tr.model._encode(inputs, pct)
        return out[0, first:first + n].float().contiguous()

    def _decode(self, rows) -> None:
        """rows (n, C) of the current segment to the decoder; the partial text and the trailing blank run afterwards"""
        import torch
        am = torch.argmax(rows, dim=-1)
        if self.tr.decoder == "beam":
            tokens, n_tok = self.decoder.feed(rows.unsqueeze(0).contiguous())[:2]
            tokens, n_tok = tokens[0, 0], n_tok[0, 0]
        else:
            tokens, n_tok = self.decoder.feed(am.to(torch.int32).unsqueeze(0).contiguous())
            tokens, n_tok = tokens[0], n_tok[0]
        blank_h = (am == self.blank).tolist()                      # the feed's one wait for the device
        n_h = max(int(n_tok), 0)
        self._partial = "".join(self.tr.labels[c] for c in tokens[:n_h].tolist())
        for is_blank in blank_h:
            self._trailing_blank = self._trailing_blank + 1 if is_blank else 0

    def _commit(self) -> None:
        self._committed.append({"start_frame": self._seg_start, "end_frame": self.frames, "text": self._partial})
        self._seg_start = self.frames
        self._partial = ""
        self._trailing_blank = 0
        self.decoder.reset()

    def _emit(self, rows) -> None:
        """the emitted rows of one window: to the decoder, cut where a segment reaches max_segment_s; the endpoint check after it"""
        if self.keep_logp:
            self._kept.append(rows)
        i = 0
        while i < rows.shape[0]:
            take = min(rows.shape[0] - i, self._seg_start + self.seg_frames - self.frames)
            self._decode(rows[i:i + take])
            self.frames += take
            i += take
            if self.frames - self._seg_start >= self.seg_frames:
                self._commit()
        if self.ep_frames and self._partial and self._trailing_blank >= self.ep_frames:
            self._commit()

    def _run(self, final: bool) -> None:
        import torch
        with torch.no_grad():
            for s0, s1, first, n in plan_windows(self._total, final, self.chunk, self.left, self.right, self.frames, self._out_frames):
                self._emit(self._window_logp(s0, s1, first, n))

    def _record(self, final: bool) -> dict:
        committed = join_texts([c["text"] for c in self._committed], self.tr.labels)
        return {"text": join_texts([committed, self._partial], self.tr.labels), "committed": committed, "partial": self._partial,
                "frames": self.frames, "final": final}

    @property
    def logp(self):
        """the emitted log-prob rows (frames, C) of the recording so far (keep_logp=True)"""
        import torch
        if not self.keep_logp:
            raise ValueError("the recogniser was built with keep_logp=False")
        return torch.cat(self._kept) if self._kept else torch.zeros(0, self.blank + 1, device=self.device)

    # ------------------------------------------------------------------------------------------ the surface
    def feed(self, samples) -> dict:
        """the next packet: f32 in [-1, 1) or int16 PCM, 16 kHz, any length, a host or device tensor, a numpy array or a list"""
        wave = self._as_wave(samples)
        i = 0
        while i < wave.numel():
            # never more at once than the buffer has room for once the spent samples are dropped
            piece = wave[i:i + self._span]
            self._append(piece)
            i += piece.numel()
            self._run(False)
        return self._record(False)

    def finish(self) -> dict:
        self._run(True)
        if self._partial or self.frames > self._seg_start:
            self._commit()
        rec = self._record(True)
        rec["segments"] = [c for c in self._committed if c["end_frame"] > c["start_frame"]]
        if self.keep_logp:
            rec["logp"] = self.logp
        self.reset()
        return rec
