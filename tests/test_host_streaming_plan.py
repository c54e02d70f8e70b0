"""The streaming window plan (streaming.plan_windows) against the independently written tests/helpers/stream_oracle.py: the
emitted frames tile the recording exactly once and in order, every window lies inside the audio received, and the plan is the
same however the audio was cut into packets.  No GPU, no torch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stream_oracle as SO  # noqa: E402

from lightning_asr_amd.streaming import plan_windows, total_frames  # noqa: E402

TOTALS = [1, 319, 320, 321, 5056, 16000, 48001, 163840]
# (chunk, left, right) in samples: the defaults, a short step, no right context, no left context, neither, one-frame steps
PARAMS = [(16000, 64000, 16000), (8000, 16000, 8000), (16000, 32000, 0), (3200, 0, 6400), (5120, 0, 0), (320, 640, 320)]
PACKETS = [1, 1600, 7777, None]


def run_packets(total, packet, chunk, left, right):
    """feeds `total` samples in packets of `packet` (None: at once), then ends the recording; every window planned on the way"""
    got, emitted, fed = [], 0, 0
    sizes = [total] if packet is None else [packet] * (total // packet) + ([total % packet] if total % packet else [])
    for i, n in enumerate(sizes):
        fed += n
        for w in plan_windows(fed, False, chunk, left, right, emitted):
            assert w[1] <= fed, (w, fed)                  # inside the audio received
            got.append(w)
            emitted += w[3]
    for w in plan_windows(total, True, chunk, left, right, emitted):
        got.append(w)
        emitted += w[3]
    assert plan_windows(total, True, chunk, left, right, emitted) == []      # the recording is done
    return got


@pytest.mark.parametrize("chunk,left,right", PARAMS)
def test_plan_matches_oracle_and_tiles_the_recording(chunk, left, right):
    for total in TOTALS:
        want = SO.plan(total, True, chunk, left, right, 0)
        assert plan_windows(total, True, chunk, left, right, 0) == want, total
        nxt = 0
        for s0, s1, first, n in want:
            assert 0 <= s0 < s1 <= total and s0 % 320 == 0, (total, s0, s1)
            assert n > 0 and first >= 0
            assert s0 // 320 + first == nxt, (total, s0, first, nxt)         # in order, no gap, no overlap
            # the window's own output has these frames: 1 + (L + 64) // 160 feature frames through the stride-2 model
            assert first + n <= ((s1 - s0 + 64) // 160) // 2 + 1, (total, s0, s1, first, n)
            nxt += n
        assert nxt == SO.recording_frames(total) == total_frames(total), (total, nxt)
        # the context a step asked for is there unless the recording's edge cuts it
        for s0, s1, first, n in want[:-1]:
            assert first * 320 == min(left, s0 + first * 320) and s1 - (s0 + (first + n) * 320) == right


@pytest.mark.parametrize("chunk,left,right", PARAMS)
def test_plan_does_not_depend_on_the_packets(chunk, left, right):
    for total in TOTALS:
        if total > 50000 and chunk < 3200:
            continue                                      # one-frame steps over ten seconds: nothing new, and slow sample by sample
        plans = {}
        for packet in PACKETS:
            if packet == 1 and total > 50000:
                continue
            plans[packet] = run_packets(total, packet, chunk, left, right)
        first = plans[None]
        for packet, p in plans.items():
            assert p == first, (total, packet)
        assert first == SO.plan(total, True, chunk, left, right, 0), total


def test_mid_stream_calls_match_the_oracle():
    chunk, left, right = 8000, 16000, 8000
    for total in (0, 15999, 16000, 23999, 24000, 100000):
        for emitted in (0, 25, 50, 75):
            for final in (False, True):
                if emitted // 25 > max(total - right, 0) // chunk:
                    continue                              # not a state a recogniser reaches: that step's audio has not arrived
                assert plan_windows(total, final, chunk, left, right, emitted) == SO.plan(total, final, chunk, left, right, emitted), \
                    (total, emitted, final)
    assert plan_windows(0, True, chunk, left, right, 0) == []


def test_bad_parameters():
    for chunk, left, right in [(0, 0, 0), (100, 0, 0), (320, 100, 0), (320, 0, -320), (-320, 0, 0)]:
        with pytest.raises(ValueError):
            plan_windows(1000, False, chunk, left, right, 0)
