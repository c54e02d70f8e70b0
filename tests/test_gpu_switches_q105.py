"""GPU tier: the A/B switches of the library (DESIGN.md §4 "Switches") on the "q105" plan - 52 units, residual blocks of five units.
The unchanged tests/switch_probe.py runs one bf16 training step + eval forward per switch in a subprocess (the switches are read once
per process), at B = 8, 160 000 samples, ragged (T' = 501: the half-tile fused depthwise forms and the sliced BN kernels).  Switches
that select other kernels must agree with the default step under tests/test_gpu_switches.py's `_close` bounds (loss 2e-3, gradient
norms per layer group 5e-2, eval checksum 5e-3, all relative); switches that only move work between launches must give the same
numbers."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (8, 160000, 1)
_BASE = {}


def _env(env_extra):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("LASR_") and k not in ("LASR_LIB_PATH",):
            del env[k]
    env.update(env_extra)
    return env


def _run(env_extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_probe.py"), "q105", "28"] + [str(a) for a in SHAPE],
                         env=_env(env_extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (env_extra, out.stderr[-2000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def _eval_probe(env_extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "q105_eval_probe.py"), str(SHAPE[0]), str(SHAPE[1])],
                         env=_env(env_extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (env_extra, out.stderr[-2000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def _base():
    if not _BASE:
        _BASE.update(_run({}))
        assert _BASE["loss"] > 0 and all(v > 0 for v in _BASE["grad_norm"].values())
        assert len(_BASE["grad_norm"]) == 13          # first_cnn, ten blocks, last_cnn2, decoder
    return _BASE


def _close(a, b, env):          # tests/test_gpu_switches.py:43-47
    assert abs(a["loss"] - b["loss"]) <= 2e-3 * abs(b["loss"]), (env, a["loss"], b["loss"])
    for k, v in b["grad_norm"].items():
        assert abs(a["grad_norm"][k] - v) <= 5e-2 * v + 1e-6, (env, k, a["grad_norm"][k], v)
    assert abs(a["eval_checksum"] - b["eval_checksum"]) <= 5e-3 * abs(b["eval_checksum"]), (env, a["eval_checksum"], b["eval_checksum"])


@pytest.mark.parametrize("switch", ["LASR_NO_FUSE", "LASR_NO_DEFER", "LASR_DW_NO_FUSED_BWD", "LASR_NO_EVAL_FOLD"])
def test_q105_kernel_switches_agree_with_the_default_paths(dev, switch):
    _close(_run({switch: "1"}), _base(), switch)


@pytest.mark.parametrize("switch", ["LASR_BN_DW_FUSE", "LASR_BN_FWD_FINALIZE", "LASR_DW_TAPS"])
def test_q105_launch_placement_switches_are_bit_identical(dev, switch):
    base = dict(_base())
    other = _run({switch: "0"})
    if switch == "LASR_BN_DW_FUSE":
        # the plan's own rule (csrc/model.hip forward_impl: a unit whose successor is a stride-1 depthwise unit of its width) hands
        # over first_cnn and every block sub-unit but the last one: each gets a BN-apply bracket of its own with the switch off
        units = _eval_probe({})["units"]
        handed = sum(1 for a, b in zip(units[:-1], units[1:]) if b != "last_cnn2")
        assert handed == 50 and len(units) == 52
        assert other["prof_brackets"]["bn"] - base["prof_brackets"]["bn"] == handed, (base["prof_brackets"], other["prof_brackets"])
        assert other["prof_brackets"]["dwconv"] == base["prof_brackets"]["dwconv"]
    base.pop("prof_brackets"); other.pop("prof_brackets")
    assert other == base, (switch, other, base)


def test_q105_eval_fold_really_runs_on_inner_units_too(dev):
    """the folded eval forward (one GEMM per block sub-unit, BatchNorm folded into its weights) makes one BN bracket fewer per folded
    unit than LASR_NO_EVAL_FOLD=1 - the 10 closing units and the 40 inner ones - and agrees with it"""
    fold, nofold = _eval_probe({}), _eval_probe({"LASR_NO_EVAL_FOLD": "1"})
    units = fold["units"]
    folded = [u for u in units if u not in ("first_cnn", "last_cnn2")]
    assert len(folded) == 50 and sum("." in u for u in folded) == 40
    assert nofold["prof_brackets"]["bn"] - fold["prof_brackets"]["bn"] == len(folded), (fold["prof_brackets"], nofold["prof_brackets"])
    assert abs(fold["eval_checksum"] - nofold["eval_checksum"]) <= 5e-3 * abs(nofold["eval_checksum"])
