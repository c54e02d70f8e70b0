"""CPU tier of the "q105" variant: the helper oracle (tests/helpers/q105_oracle.py) against the two fixtures captured from the
reference (so fixtures and helper agree without a GPU), the plan's layout and unit list through the C ABI's host-side calls, the
variant tables, and the header / library symbol check."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from oracle import ref_cpu as R                        # noqa: E402
from oracle.make_golden import checksum, golden_inputs  # noqa: E402
import q105_oracle as Q                                # noqa: E402


@pytest.mark.parametrize("mask,fname", [(True, "model_q105.npz"), (False, "model_q105_nomask.npz")])
def test_helper_oracle_matches_reference_fixture(mask, fname):
    """make_golden.check's tolerances (rtol 2e-4, atol 2e-5) on everything the fixture holds: eval and training log-probs, lengths,
    nll, the first loss, tap checksums, per-tensor gradient norms.  The helper restates the reference op for op, so on the machine
    that wrote the fixture the difference is zero; the tolerance is for another torch build's f32 summation order."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = np.load(os.path.join(ROOT, "tests", "golden", fname))
    x, tg, pct, tsz = golden_inputs()
    o = Q.OracleModel(28, mask=mask, state=Q.formula_state(28, gain=Q.GOLDEN_GAIN[mask]))
    o.training = False
    with torch.no_grad():
        lp_e = o(x, pct)
    o.training, o.keep_taps = True, True
    o.requires_grad_(True)
    lp = o(x, pct)
    t_len = R.mask_lengths(lp.size(1), pct)
    nll = R.ctc_loss_per_sample(lp, tg, t_len, tsz, 27)
    nll.mean().backward()

    def close(a, b, what):
        assert np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=2e-4, atol=2e-5), what
    close(gold["eval_logprobs"], lp_e.numpy(), "eval_logprobs")
    close(gold["logprobs"], lp.detach().numpy(), "logprobs")
    assert gold["t_lengths"].tolist() == t_len.tolist() == [101, 101, 90, 50]
    close(gold["nll"], nll.detach().numpy(), "nll")
    close(gold["losses"][0], nll.mean().item(), "loss")
    for name in ["first_cnn"] + [b[0] for b in Q.BLOCKS] + ["last_cnn2"]:
        close(gold["tap_" + name], checksum(o.taps[name]), "tap_" + name)
    norms = np.array([p.grad.norm().item() for p in o.parameters()])
    assert norms.shape == gold["grad_norms"].shape == (239,)
    assert np.abs(norms / gold["grad_norms"] - 1).max() < 5e-3
    # the quirk is in the fixtures: with mask=True there is no activation inside a block, so an inner unit's output has negative
    # values; with mask=False it has none
    inner = o.taps["block1.seq.1"]
    assert bool((inner < 0).any()) == mask


def _create(variant_id, n_class=28, mask=1, dtype=None):
    from lightning_asr_amd import _lib
    lib = _lib.load()
    cfg = _lib.ModelConfig(variant_id, n_class, 64, mask, 1, _lib.BF16 if dtype is None else dtype)
    h = C.c_void_p()
    rc = lib.lasr_model_create(C.byref(cfg), C.byref(h))
    return lib, h, rc


def test_plan_layout_and_units_on_the_host():
    """lasr_model_create / tensor_info / unit_info are host code: the layout is the reference state dict's (425 entries,
    11 669 340 parameters at 28 classes), the plan has 52 units, a block's closing unit keeps the block's name"""
    from lightning_asr_amd import _lib
    lib, h, rc = _create(_lib.VARIANT["q105"])
    assert rc == 0
    try:
        n = lib.lasr_model_tensor_info(h, -1, None, 0, None, None, None, None)
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        ndim, kind, off = C.c_int32(), C.c_int32(), C.c_int64()
        got = []
        for i in range(n):
            lib.lasr_model_tensor_info(h, i, name, 256, shape, C.byref(ndim), C.byref(kind), C.byref(off))
            got.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
        assert got == [(k, tuple(s)) for k, s in Q.state_shapes(28)]
        assert n == 425 and lib.lasr_model_param_elems(h) == 11669340
        nu = lib.lasr_model_num_units(h)
        units = []
        for i in range(nu):
            assert lib.lasr_model_unit_info(h, i, name, 256) == 0
            units.append(name.value.decode())
        assert units == ["first_cnn"] + [u[0] for u in Q.unit_table()] + ["last_cnn2"] and nu == 52
        # taps: the suffix forms for both kinds of unit name (offsets into a workspace nobody has to allocate for this)
        shp = (C.c_int64 * 3)()
        assert lib.lasr_model_workspace_bytes(h, 4, 201, 12) > 0
        for tap, c in (("block3", 512), ("block3.y", 512), ("block3.y2", 512), ("block3.u", 256), ("block3.seq.2", 256),
                       ("block3.seq.2.y", 256), ("block3.seq.2.u", 256), ("block52.seq.0", 512)):
            assert lib.lasr_model_tap(h, tap.encode(), 4, 201, 12, shp) >= 0, tap
            assert tuple(shp) == (4, 101, c), tap
        assert lib.lasr_model_tap(h, b"block3.seq.2.y2", 4, 201, 12, shp) < 0          # inner units have no residual branch
    finally:
        lib.lasr_model_destroy(h)


def test_existing_variants_keep_their_plan():
    """the other variants' unit lists and workspace sizes are what they were (recorded from the parent revision)"""
    from lightning_asr_amd import _lib
    # variant: units, state-dict entries, parameters, bf16 workspace bytes at (B, T_in, S_max) = (4, 201, 12) and (32, 1001, 100)
    want = {"plain": (15, 184, 5044572, 437023232, 1992840960), "context": (16, 205, 5796812, 491417344, 2290383872),
            "context_se": (16, 235, 6435788, 493083904, 2294770688), "q105": (52, 425, 11669340, 920903168, 5029380864)}
    for variant, (nu, nt, npar, ws_small, ws_cfg2) in want.items():
        lib, h, rc = _create(_lib.VARIANT[variant])
        assert rc == 0
        try:
            assert lib.lasr_model_num_units(h) == nu
            assert lib.lasr_model_tensor_info(h, -1, None, 0, None, None, None, None) == nt
            assert lib.lasr_model_param_elems(h) == npar
            assert lib.lasr_model_workspace_bytes(h, 4, 201, 12) == ws_small
            assert lib.lasr_model_workspace_bytes(h, 32, 1001, 100) == ws_cfg2
        finally:
            lib.lasr_model_destroy(h)


def test_variant_tables_and_unknown_variant():
    from lightning_asr_amd import _lib
    from lightning_asr_amd.train import MODEL_FILES, _model_class
    assert _lib.VARIANT["q105"] == 3 and set(_lib.VARIANT) == set(MODEL_FILES)
    assert MODEL_FILES["q105"] == "QuartNet105"
    cls = _model_class("q105")
    assert cls.__name__ == "MyModel2" and cls.variant == "q105"
    with pytest.raises(KeyError):
        _model_class("q15x5")
    with pytest.raises(KeyError):
        _lib.VARIANT["q15x5"]
    lib, h, rc = _create(4)
    assert rc == -1 and b"bad config" in lib.lasr_last_error()
    lib, h, rc = _create(-1)
    assert rc == -1


def test_header_and_library_export_the_same_symbols():
    import re
    from lightning_asr_amd import _lib
    text = open(os.path.join(ROOT, "include", "lasr.h")).read()
    assert "LASR_VARIANT_Q105 = 3" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lasr_[a-z0-9_]+)\s*\(", text)))
    lib = C.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    assert set(_lib.SIGNATURES) == set(syms)
