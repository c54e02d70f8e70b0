"""An independent statement of the streaming window plan (lightning_asr_amd/streaming.py plan_windows), for
tests/test_host_streaming_plan.py.  It never looks at one call's arguments alone: it lists every window of the whole recording
from its first sample, with the frame each emits first counted on the RECORDING's frame axis (a recording of L samples has
((L + 64) // 160) // 2 + 1 frames: the feature frames 1 + (L + 64) // 160 through the model's stride-2 convolution), and then
keeps the windows a call is still owed."""

SAMPLES_PER_FRAME = 320


def recording_frames(total):
    return ((total + 64) // 160) // 2 + 1 if total > 0 else 0


def all_windows(total, final, chunk, left, right):
    """[(first sample, end sample, first emitted frame of the recording, frames emitted)] for the audio [0, total)"""
    per = chunk // SAMPLES_PER_FRAME
    out = []
    step = 0
    while chunk * (step + 1) + right <= total:
        lo = step * chunk - left
        out.append((lo if lo > 0 else 0, chunk * (step + 1) + right, step * per, per))
        step += 1
    if final and total > 0:
        lo = step * chunk - left
        lo = lo if lo > 0 else 0
        if lo >= total:                       # no sample left for the last frame's window: one frame of audio before the end
            lo = total - SAMPLES_PER_FRAME
        rest = recording_frames(total) - step * per
        if rest > 0:
            out.append((lo, total, step * per, rest))
    return out


def plan(total, final, chunk, left, right, emitted_frames):
    """plan_windows' answer: the windows whose frames are not emitted yet, the first frame as an index into the window's output"""
    return [(lo, hi, g - lo // SAMPLES_PER_FRAME, n) for lo, hi, g, n in all_windows(total, final, chunk, left, right)
            if g >= emitted_frames]
