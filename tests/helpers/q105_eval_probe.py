"""Helper of tests/test_gpu_switches_q105.py: one bf16 EVAL forward of the q105 plan under whatever LASR_* switches the environment
carries (tests/switch_probe.py brackets the training step only); prints a JSON line with the bracket counts per kernel class of that
forward, the plan's unit names and a checksum of the log-probs."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from lightning_asr_amd import _lib  # noqa: E402
from lightning_asr_amd.engine import NativeModel  # noqa: E402
from lightning_asr_amd.step import TrainStep  # noqa: E402


def main():
    B, L = int(sys.argv[1]), int(sys.argv[2])
    dev = torch.device("cuda:0")
    wave, _, _ = bench.synth_batch(B, L, 20, 77, dev, 27)
    sl = torch.tensor([L - (i % 5) * (L // 14) for i in range(B)], dtype=torch.int32, device=dev)
    wave = wave * (torch.arange(L, device=dev).unsqueeze(0) < sl.unsqueeze(1))
    m = NativeModel("q105", 28, mask=True, act="relu", dtype=torch.bfloat16, device=dev)
    m.init_parameters(seed=1)
    ts = TrainStep(m, 1e-2, 1e-3)
    feats, pct = ts.features(wave, sl)
    lib = _lib.load()
    m.forward(feats, pct, training=False)            # (sizes the workspace outside the brackets)
    torch.cuda.synchronize()
    lib.lasr_prof_enable(1)
    lp, am = m.forward(feats, pct, training=False)
    torch.cuda.synchronize()
    lib.lasr_prof_enable(0)
    ms = (C.c_double * 8)(); fl = (C.c_double * 8)(); by = (C.c_double * 8)(); cnt = (C.c_int64 * 8)()
    _lib.check(lib.lasr_prof_collect(ms, fl, by, cnt), "lasr_prof_collect")
    print(json.dumps({"prof_brackets": {k: int(cnt[i]) for i, k in enumerate(bench.PROF_KINDS)}, "units": m.unit_names(),
                      "eval_checksum": float(lp.double().abs().mean()), "eval_max": float(lp.double().abs().max()),
                      "argmax_sum": int(am.long().sum())}))


if __name__ == "__main__":
    main()
