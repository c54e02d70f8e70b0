"""The depthwise kernels (csrc/conv.hip) called directly through lasr_dwconv_fwd / lasr_dwconv_wgrad / lasr_dwconv_bwd_fused and held
to the plain f64 CPU reference of tests/helpers/dwconv_cases.py (itself checked against a triple loop in
tests/test_host_dwconv_cases.py) - every kernel form, every template instance, both sides of every tile edge and dispatch threshold.

Exact pass.  Small-integer operands (helpers/dwconv_cases.py "int" and "pos") make every product and every partial sum an integer
below 256 resp. 2^24, exact in bf16 resp. f32 in any order of summation: every op of every case must be torch.equal to the
reference, in the op's storage type.  The condition is asserted on each case's own reference before the comparison.

Which form ran.  lasr_dwconv_plan (the launchers' own dispatch code, launching nothing) labels every failure, and the coverage
assertions hold the table to it: under default switches it reaches all eight <NKS, NSET> forward instances, both weight-gradient
forms (time splits 1 and 2), both unified backward instances with a time-split grid, idle workgroups in the padded grid and more
tiles than workgroups, the two-kind grid the narrow windows take, the VALU fall-backs of the wide ones and both strided instances;
under each switch set (a fresh process each: tests/helpers/dwconv_probe.py) the named alternative form is the one chosen.

Random pass (in process and in every child): one case per distinct plan, randn operands rounded to the tensor's dtype, at the
tolerances tests/test_gpu_ops.py already holds these ops to - bf16 forward / data gradient max_rel < 4e-3, weight gradient
< 2e-5 * scale + 1e-6, f32 forward 2e-6, f32 weight gradient 2e-5.  The worst figure per form goes to the run's measured record
(conftest.record_measured, names "dwconv_parity | switches | form"; profiles/dwconv_parity_measured.json keeps a copy of those
entries); the gates are not derived from it.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import record_measured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import dwconv_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH_SETS = [
    {"LASR_DWCONV_FMA": "1"},          # forward / data gradient: dwconv_s1_kernel<bf16_t>
    {"LASR_DWCONV_DOT2": "1"},         # ... dwconv_s1_bf16_kernel (also the default fall-back of k > 113)
    {"LASR_DWWGRAD_VALU": "1"},        # weight gradient: dwconv_wgrad_s1_kernel<bf16_t>
    {"LASR_DW_UNI": "0"},              # backward: dwconv_bwd_s1_mfma_kernel (two kinds of workgroup in one grid)
    {"LASR_DW_UNI": "64"},             # backward: the 64-channel unified kernel at every k
    {"LASR_DW_NO_FUSED_BWD": "1"},     # backward: the two launches
    {"LASR_DWCONV_NO_HALF": "1"},      # forward: full 512-frame tiles only (tile loops with gridDim.z = 1)
    {"LASR_DWWGRAD_ZSPLIT": "8"},      # weight gradient: up to 8 time splits per utterance
]

_REFS = {}


def _ref(case, kind=None):
    key = case.name + (D.RAND if kind == "rand" else "")
    if key not in _REFS:
        _REFS[key] = D.reference(case, kind)
    return _REFS[key]


def _record(figures, who):
    """the random pass's worst figure per kernel form into the run's measured record (conftest.record_measured)"""
    for form, v in sorted(figures.items()):
        record_measured("dwconv_parity | %s | %s" % (who, form), float("%.3e" % v))


def test_table_reaches_every_form_under_default_switches():
    plans = {c.name: D.plan_of(c) for c in D.TABLE}
    assert D.coverage_gaps(plans) == []


@pytest.mark.parametrize("name", [c.name for c in D.TABLE])
def test_exact_on_integer_operands(dev, name):
    case = D.BY_NAME[name]
    ref = _ref(case)
    ok, ymax, wmax = D.exactness(ref)
    assert ok, ("the operands do not meet the exactness condition", name, ymax, wmax)
    bad = D.exact_pass(case, dev, ref)
    lines = ["%s %s [%s]: %d elements wrong, first at %s: got %r, want %r" % (name, m["op"], m["form"], m["wrong"], tuple(m["first"]),
                                                                              m["got"], m["want"]) for m in bad]
    assert not bad, "\n".join(lines + ["plan: %r" % (D.plan_of(case),)])


def test_random_operands_at_the_project_tolerances(dev):
    figures, fails = D.rand_pass(D.TABLE, dev, lambda c: _ref(c, "rand"))
    _record(figures, "default")
    assert not fails, fails


def _child(env_extra, refs_path):
    env = dict(os.environ)
    for k in list(env):
        if k.startswith("LASR_") and k not in ("LASR_LIB_PATH",):
            del env[k]
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "dwconv_probe.py"), "--refs", refs_path], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (env_extra, out.returncode, out.stderr[-2000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_switch_forms_in_fresh_processes(dev, tmp_path):
    """every alternative form the LASR_DW* switches select, on the bf16 stride-1 part of the table and the stride-2 cases: the
    child's own plan shows the intended form, every op is exact on the integer operands and the random pass holds.  The children
    run one after the other; one that does not exit cleanly ends the test there."""
    cases = D.worker_cases()
    refs = {c.name: _ref(c) for c in cases}
    for c in D.one_case_per_plan(cases):        # the random pass's picks under default switches; a child whose switches make it pick
        refs[c.name + D.RAND] = _ref(c, "rand")  # another case computes that reference itself
    path = str(tmp_path / "dwconv_refs.pt")
    D.save_refs(path, refs)
    for env in SWITCH_SETS:
        res = _child(env, path)
        assert set(res["plans"]) == {c.name for c in cases}
        assert D.switch_gaps(env, res["plans"]) == [], env
        assert res["not_exact"] == [], env
        assert res["mismatches"] == [], (env, len(res["mismatches"]), res["mismatches"][:8],
                                         [res["plans"][m["case"]] for m in res["mismatches"][:2]])
        assert res["rand_fail"] == [], (env, res["rand_fail"])
        _record(res["rand"], " ".join("%s=%s" % kv for kv in env.items()))


def _sentinel(shape, dtype, dev):
    return torch.full(shape, 7.0, dtype=dtype, device=dev)


def test_refused_shapes_return_an_error_and_write_nothing(dev):
    from lightning_asr_amd import _lib
    lib = _lib.load()
    B, T = 2, 40
    for what, dtype, C, k, stride, flip in [("even k", torch.float32, 8, 4, 1, 0), ("k = 129", torch.float32, 8, 129, 1, 0),
                                            ("stride 3", torch.float32, 8, 5, 3, 0), ("flip with stride 2", torch.float32, 8, 5, 2, 1),
                                            ("bf16 stride 1 with C = 12", torch.bfloat16, 12, 5, 1, 0),
                                            ("even k, bf16", torch.bfloat16, 64, 32, 1, 0), ("k = 129, bf16", torch.bfloat16, 64, 129, 1, 0)]:
        code = _lib.BF16 if dtype == torch.bfloat16 else _lib.F32
        x = torch.ones(B, T, C, dtype=dtype, device=dev)
        w = torch.ones(C, k, dtype=torch.float32, device=dev)
        y = _sentinel((B, T, C), dtype, dev)
        dw = _sentinel((C, k), torch.float32, dev)
        nb = max(int(lib.lasr_dwconv_wgrad_workspace_bytes(B, T, C, min(k, 127))), 256) * 2
        ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.lasr_dwconv_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), code, B, T, C, k, stride, flip, st)
        assert rc != 0 and lib.lasr_last_error(), ("lasr_dwconv_fwd", what, rc)
        if not flip:
            rc = lib.lasr_dwconv_wgrad(x.data_ptr(), x.data_ptr(), dw.data_ptr(), code, B, T, C, k, stride, ws.data_ptr(), nb, st)
            assert rc != 0, ("lasr_dwconv_wgrad", what, rc)
            plan = _lib.DwconvPlan()
            assert lib.lasr_dwconv_plan(B, T, C, k, stride, code, ctypes.byref(plan)) != 0, ("lasr_dwconv_plan", what)
        if stride == 1:
            npart = ctypes.c_int(-5)
            rc = lib.lasr_dwconv_bwd_fused(x.data_ptr(), x.data_ptr(), w.data_ptr(), None, y.data_ptr(), code, B, T, C, k, ws.data_ptr(), nb,
                                           ctypes.byref(npart), st)
            assert rc != 0 and npart.value == -5, ("lasr_dwconv_bwd_fused", what, rc, npart.value)
        torch.cuda.synchronize()
        assert bool((y == 7).all()) and bool((dw == 7).all()) and bool((ws == 0).all()), (what, "a refused call wrote its output")
