"""Generate tests/golden/pseudo_confidence.npz by running the REFERENCE's utterance confidences (ssl_codec/utils.py: sum_logprob
and seq_sum_logprob_np, loaded by path from a reference checkout, development container only) on seeded log-probs.

    python tools/make_pseudo_golden.py <reference checkout>

Only seeds, shapes, lens and the reference's OUTPUTS are stored (as float64: sum_logprob sums Python floats; the running sum of
seq_sum_logprob_np is float32 under numpy's scalar promotion, Python float + np.float32 -> np.float32, so its gate is wider);
the inputs are regenerated from the seed on both sides (tests/helpers/greedy_conf_oracle.make_logp).  Never imported by a test.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import greedy_conf_oracle as O  # noqa: E402

# name -> (seed, B, T, C, blank_bias, lens): the blank (the last class) wins a good share of the frames, some lens < T
CASES = {
    "c28": (101, 3, 50, 28, 5.0, [50, 37, 1]),
    "c4334": (202, 2, 20, 4334, 9.0, [20, 13]),
}


def main(ref_root: str) -> None:
    spec = importlib.util.spec_from_file_location("ref_ssl_utils", os.path.join(ref_root, "ssl_codec", "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"cases": np.array(sorted(CASES))}
    for name, (seed, B, T, C, bias, lens) in CASES.items():
        logp = O.make_logp(seed, B, T, C, C - 1, bias)
        blank_frames = int((logp.argmax(-1) == C - 1).sum())
        assert 0 < blank_frames < B * T, (name, blank_frames)
        f64 = np.asarray(ref.sum_logprob(torch.from_numpy(logp), list(lens)), dtype=np.float64)
        f32 = np.asarray([float(ref.seq_sum_logprob_np((b, logp[b], lens[b]))[1]) for b in range(B)], dtype=np.float64)
        out[name + "_shape"] = np.array([seed, B, T, C], dtype=np.int64)
        out[name + "_blank_bias"] = np.float64(bias)
        out[name + "_lens"] = np.array(lens, dtype=np.int32)
        out[name + "_sum_logprob"] = f64
        out[name + "_seq_sum_logprob_np"] = f32
        print(name, "blank frames %d / %d" % (blank_frames, B * T), f64, f32)
    path = os.path.join(ROOT, "tests", "golden", "pseudo_confidence.npz")
    np.savez(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
